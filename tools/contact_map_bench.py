#!/usr/bin/env python3
"""The contact map's pass (ig_contact_map, csrc/ig_kernels_map.cuh) timed at the headline shapes -> profiles/r07_contact_map.json.

Per config (cfg3, cfg3_late), after a number of batch moves, max_side = 2048, median of 20 after 3 warm-ups:
  (a) the pass as shipped: zero the image, k_contact_map with equal destinations combined inside the wave, k_map_mirror
      (hipEvents around it on the library's stream: ig_debug_contact_map_time);
  (b) the same kernel with the combining switched off by its template flag: one atomic per contact end -- the yardstick;
  (c) the host restatement of tests/test_hip_contact_map.py on the same contacts: numpy, the contacts split over 16 threads.
and the whole ``sampler.contact_map`` call on the host clock (order on the host, pixel table, pass, 32 MB copy back).

  python tools/contact_map_bench.py [--configs cfg3,cfg3_late] [--out profiles/r07_contact_map.json]
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/contact_map_bench.py --trace-run cfg3     (a few passes only)
  python tools/contact_map_bench.py --merge-stats DIR/.../run_results.db --out profiles/r07_contact_map.json
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np

import _report_bench as kit

MAX_SIDE = 2048
THREADS = 16


def host_map(prob, order, max_side):
    """the image on the host: positions from the order, np.bincount over THREADS slices of the contacts, symmetrised"""
    T = order.size
    where = np.full(prob.n_sub_frags, -1, np.int64)
    where[order] = np.arange(T)
    b = max(1, -(-T // max_side))
    side = -(-T // b)
    px = np.where(where >= 0, where // b, -1)
    cuts = np.linspace(0, prob.coo_row.size, THREADS + 1).astype(np.int64)

    def part(k):
        r, c, v = (a[cuts[k]:cuts[k + 1]] for a in (prob.coo_row, prob.coo_col, prob.coo_cnt))
        pi, pj = px[r], px[c]
        ok = (pi >= 0) & (pj >= 0)
        return np.bincount(pi[ok] * side + pj[ok], weights=v[ok], minlength=side * side)

    with ThreadPoolExecutor(THREADS) as ex:
        upper = sum(ex.map(part, range(THREADS))).astype(np.int64).reshape(side, side)
    return upper + upper.T


def measure(cfg, moves, reps, warmup):
    prob, s = kit.make_sampler(cfg, moves)
    Z, M = int(prob.coo_row.size), int(prob.n_sub_frags)
    out = dict(config=cfg, moves_before=moves, contacts=Z, sub_fragments=M, max_side=MAX_SIDE)
    image, b = s.contact_map(MAX_SIDE)
    side = image.shape[0]
    out.update(bin=int(b), side=int(side), image_bytes=int(image.nbytes))
    for key, combine in (("pass_combined_us", True), ("pass_one_atomic_per_end_us", False)):
        ms, tot = s.ctx.debug_contact_map_time(MAX_SIDE, combine=combine, n=warmup + reps)
        assert tot == int(image.sum())
        kit.put_times(out, key, ms[warmup:])
    out["whole_call_host_clock_ms"] = kit.host_clock_ms(lambda: s.contact_map(MAX_SIDE), reps, warmup)
    order = s.ctx.contact_map_order()
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = host_map(prob, order, MAX_SIDE)
        t.append(time.perf_counter() - t0)
    assert np.array_equal(want, image)
    out["host_numpy_%d_threads_ms" % THREADS] = round(1e3 * float(np.median(t)), 1)
    # bytes the pass reads: row (4) + column and count (8) per contact, two 4-byte gathers from the pixel table (L2-resident:
    # counted once per table), and what it writes: the zeroed image, the mirror's read and write of it
    out["bytes_streamed"] = 12 * Z + 4 * M
    out["bytes_image_traffic"] = 3 * int(image.nbytes)
    sec = out["pass_combined_us"] * 1e-6
    out["contacts_per_second"] = round(Z / sec, 0)
    out["streamed_GB_per_second"] = round(out["bytes_streamed"] / sec / 1e9, 1)
    s.free_gpu()
    return out


def merge_stats(db_path, out_path):
    import sqlite3

    db = sqlite3.connect(db_path)
    cur = db.cursor()
    tabs = [r[0] for r in cur.execute("select name from sqlite_master where type='table'")]
    kd = [t for t in tabs if "kernel_dispatch" in t][0]
    ks = [t for t in tabs if "kernel_symbol" in t][0]
    rows = list(cur.execute(
        f"select s.kernel_name, count(*), avg(d.end-d.start), min(d.end-d.start), max(d.end-d.start), max(s.arch_vgpr_count), "
        f"max(s.sgpr_count), max(d.group_segment_size) from {kd} d join {ks} s on d.kernel_id=s.id "
        f"where s.kernel_name like '%k_contact_map%' or s.kernel_name like '%k_map_%' group by s.kernel_name order by 3 desc"))
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["kernel_trace_stats"] = dict(
        command="rocprofv3 --kernel-trace --stats -- python tools/contact_map_bench.py --trace-run cfg3 (one MI355X)",
        kernels=[dict(name=r[0], calls=r[1], avg_us=round(r[2] / 1e3, 2), min_us=round(r[3] / 1e3, 2), max_us=round(r[4] / 1e3, 2),
                      vgprs=r[5], sgprs=r[6], lds_bytes=r[7]) for r in rows])
    json.dump(doc, open(out_path, "w"), indent=1)
    for k in doc["kernel_trace_stats"]["kernels"]:
        print(k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg3,cfg3_late")
    ap.add_argument("--moves", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles", "r07_contact_map.json"))
    ap.add_argument("--trace-run", default=None, help="a few passes of both forms at this config, for a run under rocprofv3")
    ap.add_argument("--merge-stats", default=None, help="a rocprofv3 sqlite database of a --trace-run: its map kernels go into --out")
    a = ap.parse_args()
    if a.merge_stats:
        return merge_stats(a.merge_stats, a.out)
    if a.trace_run:
        prob, s = kit.make_sampler(a.trace_run, a.moves)
        for combine in (True, False):
            ms, _ = s.ctx.debug_contact_map_time(MAX_SIDE, combine=combine, n=8)
            print("combine", combine, "median %.1f us" % (1e3 * float(np.median(ms[3:]))))
        s.free_gpu()
        return
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc["what"] = ("the contact map's pass at max_side 2048 on one MI355X: median of %d after %d warm-ups, hipEvents around zero + "
                   "k_contact_map + k_map_mirror (tools/contact_map_bench.py); host figures: numpy on this box's CPUs, %d threads"
                   % (a.reps, a.warmup, THREADS))
    doc["results"] = [measure(cfg, a.moves, a.reps, a.warmup) for cfg in a.configs.split(",") if cfg]
    kit.write_doc(doc, a.out, show=doc["results"])


if __name__ == "__main__":
    main()
