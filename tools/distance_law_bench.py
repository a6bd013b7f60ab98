#!/usr/bin/env python3
"""The distance law's passes (ig_distance_law, csrc/ig_kernels_law.cuh) timed at the headline shapes -> profiles/r08_distance_law.json.

Per config (cfg3, cfg3_late), built from coo=, after a number of batch moves, under the default geometric edges and under the
estimate's linear ones; median of 20 after 3 warm-ups, hipEvents around zero + kernel (ig_debug_distance_law_time):
  (a) the observed pass as shipped: a histogram per workgroup in LDS, flushed once;
  (b) the same kernel with the privatisation switched off by its template flag: one global atomic per contact -- the yardstick;
  (c) the pairs pass;
  (d) what a user has without the pass: ig_debug_tables downloaded + a vectorised numpy histogram of the observed part, on the host
      clock; and the whole ``ctx.distance_law`` call on the host clock.

  python tools/distance_law_bench.py [--configs cfg3,cfg3_late] [--out profiles/r08_distance_law.json]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np

import _report_bench as kit


def host_observed(s, prob, edges):
    """the numpy alternative: the tables from the device, every contact binned on the host (every contig placed, as in the
    synthetic problems)"""
    dist, contig, stot, _, _ = s.ctx.debug_tables()
    row, col, cnt = prob.coo_row, prob.coo_col, prob.coo_cnt
    lin = (contig[row] == contig[col]) & (stot[row] == 0)
    sep = np.abs(dist[row[lin]] - dist[col[lin]])
    b = np.searchsorted(edges, sep, side="right") - 1
    inside = (b >= 0) & (b < edges.size - 1)
    return np.bincount(b[inside], weights=cnt[lin][inside].astype(np.float64), minlength=edges.size - 1).astype(np.int64)


def measure(cfg, moves, reps, warmup):
    from instagraal_amd import distance_law as dlaw

    prob, s = kit.make_sampler(cfg, moves)
    Z, M = int(prob.coo_row.size), int(prob.n_sub_frags)
    longest = float(s.ctx.debug_tables()[0].max())
    rows = []
    for label, edges in (("geometric_default", dlaw.default_edges(s.mean_kb(), longest)), ("linear_60_x_1kb", np.arange(0, 61, dtype=np.float32)),
                         ("linear_4096_bins", np.linspace(0, longest * 1.01, 4097).astype(np.float32))):
        out = dict(config=cfg, moves_before=moves, contacts=Z, sub_fragments=M, edges=label, bins=int(edges.size - 1))
        law = s.ctx.distance_law(edges)
        assert dlaw.observed_total(law) == int(prob.coo_cnt.astype(np.int64).sum()) and dlaw.pairs_total(law) == law["placed_pairs"]
        ms_a, ms_p, ck_a = s.ctx.debug_distance_law_time(edges, privatised=True, n=warmup + reps)
        ms_b, _, ck_b = s.ctx.debug_distance_law_time(edges, privatised=False, n=warmup + reps, pairs=False)
        assert ck_a == ck_b
        for key, ms in (("observed_privatised_us", ms_a), ("observed_one_atomic_per_contact_us", ms_b), ("pairs_us", ms_p)):
            kit.put_times(out, key, ms[warmup:])
        out["whole_call_host_clock_ms"] = kit.host_clock_ms(lambda: s.ctx.distance_law(edges), reps, warmup)
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = host_observed(s, prob, edges)
            t.append(time.perf_counter() - t0)
        assert np.array_equal(want, law["observed"])
        out["host_numpy_observed_ms"] = round(1e3 * float(np.median(t)), 1)
        out["bytes_streamed"] = 12 * Z + 16 * M  # row + (column, count) per contact; the 16-byte records once (gathers: L2)
        out["streamed_GB_per_second"] = round(out["bytes_streamed"] / (out["observed_privatised_us"] * 1e-6) / 1e9, 1)
        rows.append(out)
    s.free_gpu()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg3,cfg3_late")
    ap.add_argument("--moves", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles", "r08_distance_law.json"))
    a = ap.parse_args()
    doc = dict(what=("the distance law's passes on one MI355X: median of %d after %d warm-ups, hipEvents around zero + kernel "
                     "(tools/distance_law_bench.py); host figures: numpy on this box's CPUs, one thread, on the host clock" % (a.reps, a.warmup)))
    doc["results"] = [r for cfg in a.configs.split(",") if cfg for r in measure(cfg, a.moves, a.reps, a.warmup)]
    kit.write_doc(doc, a.out, show=doc["results"])


if __name__ == "__main__":
    main()
