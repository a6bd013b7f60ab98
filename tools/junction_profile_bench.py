#!/usr/bin/env python3
"""The junction profile's passes (ig_junction_profile, csrc/ig_kernels_junc.cuh) timed at the headline shapes
-> profiles/r09_junction_profile.json.

Per config (cfg3, cfg3_late), built from coo=, after a number of batch moves, at windows of 64 and 1024 positions; median of 20
after warm-ups, hipEvents around each pass (ig_debug_junction_profile_time; (a) and (b) alternate in four blocks of 3 warm-ups + 5):
  (a) the observed pass with equal + ends combined inside the wave;
  (b) the same kernel with the combining switched off by its template flag: one atomic per contact end -- the yardstick;
  (c) the model pass; (d) the scan of the three arrays;
  (e) for orientation k_law_observed on the same handle (default edges), which streams the same bytes;
  and the whole ``ctx.junction_profile`` call on the host clock.
The combined form ships only if its median is not above the yardstick's at both shapes (every window measured); the file says which
form the library was built with (JUNC_SHIP_COMBINE in csrc/ig_host_junc.inc) and whether that is what the figures ask for.

  python tools/junction_profile_bench.py [--configs cfg3,cfg3_late] [--out profiles/r09_junction_profile.json]
"""
import argparse
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import numpy as np

import _report_bench as kit


def measure(cfg, moves, reps, warmup, windows):
    from instagraal_amd import distance_law as dlaw, junction_profile as jp

    prob, s = kit.make_sampler(cfg, moves)
    Z, M = int(prob.coo_row.size), int(prob.n_sub_frags)
    total = int(prob.coo_cnt.astype(np.int64).sum())
    edges = dlaw.default_edges(s.mean_kb(), float(s.ctx.debug_tables()[0].max()))
    ms_law, _, _ = s.ctx.debug_distance_law_time(edges, privatised=True, n=warmup + reps, pairs=False)
    rows = []
    for w in windows:
        out = dict(config=cfg, moves_before=moves, contacts=Z, sub_fragments=M, window=w)
        prof = s.ctx.junction_profile(w)
        assert jp.observed_total(prof) == total and prof["spanned_observed"] == int(prof["observed"].sum())
        out.update(n_placed=prof["n_placed"], internal_junctions=prof["internal_junctions"],
                   in_window_share_of_counts=round(prof["in_window_observed"] / total, 4))
        # the two forms of the observed pass alternate in blocks (other work shares the machine: a drift hits both alike)
        def observed(combine):
            def timed(n):
                ms, _, _, ck = s.ctx.debug_junction_profile_time(w, combine=combine, n=n, model=False, scan=False)
                return ms, ck
            return timed

        ms_a, ms_b = kit.alternate(observed(True), observed(False), reps, warmup)
        _, ms_m, ms_s, _ = s.ctx.debug_junction_profile_time(w, combine=True, n=warmup + reps)
        ms_m, ms_s, ms_l = ms_m[warmup:], ms_s[warmup:], ms_law[warmup:]
        out["timed_repetitions"] = int(ms_a.size)
        for key, ms in (("observed_combined_us", ms_a), ("observed_one_atomic_per_end_us", ms_b), ("model_us", ms_m), ("scan_us", ms_s),
                        ("law_observed_privatised_us", ms_l)):
            kit.put_times(out, key, ms)
        out["whole_call_host_clock_ms"] = kit.host_clock_ms(lambda: s.ctx.junction_profile(w), reps, warmup)
        out["bytes_streamed"] = 12 * Z + 16 * M  # row + (column, count) per contact; the 16-byte records once (gathers: L2)
        rows.append(out)
    s.free_gpu()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg3,cfg3_late")
    ap.add_argument("--windows", default="64,1024")
    ap.add_argument("--moves", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_junction_profile.json"))
    a = ap.parse_args()
    doc = dict(what=("the junction profile's passes on one MI355X: median of %d timed repetitions behind %d warm-ups, hipEvents around each pass "
                     "(the observed pass: zero + kernel; its two forms alternate in four blocks, each behind its own warm-ups) "
                     "(tools/junction_profile_bench.py)" % (a.reps, a.warmup)))
    windows = [int(w) for w in a.windows.split(",") if w]
    doc["results"] = [r for cfg in a.configs.split(",") if cfg for r in measure(cfg, a.moves, a.reps, a.warmup, windows)]
    ok = all(r["observed_combined_us"] <= r["observed_one_atomic_per_end_us"] for r in doc["results"])
    kit.ship_verdict(doc, ok, bool(kit.shipped_flag("ig_host_junc.inc", "JUNC_SHIP_COMBINE")))
    kit.write_doc(doc, a.out)


if __name__ == "__main__":
    main()
