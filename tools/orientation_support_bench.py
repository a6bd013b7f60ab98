#!/usr/bin/env python3
"""The orientation support's passes (ig_orientation_support, csrc/ig_kernels_orient.cuh) timed at the headline shapes
-> profiles/r14_orientation_support.json.

Per config (cfg3, cfg3_late), built from coo=, after a number of batch moves, at bin and block level, at windows of 8 and 1024
positions; median of 20 after warm-ups, hipEvents around each pass (ig_debug_orientation_support_time; (a) and (b) alternate in four
blocks of 3 warm-ups + 5):
  (a) the observed pass with equal row ends combined inside the wave;
  (b) the same kernel with the combining switched off by its template flag: one atomic per counted end -- the yardstick;
  (c) the model pass as shipped (a wave per segment, a workgroup beyond ORIENT_WAVE_PAIRS terms);
  (d) for orientation k_junc_observed (one atomic per end) on the same handle at the same window, which streams the same bytes;
  and the whole ``ctx.orientation_support`` call on the host clock.
The combined form ships only if its median is not above the yardstick's at both shapes (every level and window measured); the file
says which form the library was built with (ORIENT_SHIP_COMBINE in csrc/ig_host_orient.inc) and whether that is what the figures
ask for.

  python tools/orientation_support_bench.py [--configs cfg3,cfg3_late] [--out profiles/r14_orientation_support.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import numpy as np

import _report_bench as kit


def measure(cfg, moves, reps, warmup, windows, levels):
    from instagraal_amd import orientation_support as osup

    prob, s = kit.make_sampler(cfg, moves)
    Z, M = int(prob.coo_row.size), int(prob.n_sub_frags)
    total = int(prob.coo_cnt.astype(np.int64).sum())
    rows = []
    for level in levels:
        for w in windows:
            out = dict(config=cfg, moves_before=moves, contacts=Z, sub_fragments=M, level=level, window=w)
            res = s.orientation_support(level=level, window=w)
            f, l = res["first"], res["last"]
            assert osup.observed_total(res) == total and res["entries_observed"] == int(res["observed"].sum())
            out.update(n_placed=res["n_placed"], n_seg=res["n_seg"], n_judged=res["n_judged"], counted_share_of_counts=round(res["counted"] / total, 4),
                       keep_above_flip=int((res["keep"] > res["flip"]).sum()), flip_above_keep=int((res["flip"] > res["keep"]).sum()),
                       model_terms=int(2 * res["pairs"][res["status"] == 0].sum()),
                       workgroup_segments=int((2 * res["pairs"][res["status"] == 0] > 4096).sum()))
            # the two forms of the observed pass alternate in blocks (other work shares the machine: a drift hits both alike)
            ms_a, ms_b = kit.alternate(lambda n: s.ctx.debug_orientation_support_time(w, f, l, which="observed", form="combined", n=n),
                                       lambda n: s.ctx.debug_orientation_support_time(w, f, l, which="observed", form="atomic", n=n), reps, warmup)
            ms_m, _ = s.ctx.debug_orientation_support_time(w, f, l, which="model", form="default", n=warmup + reps)
            ms_j, _, _, _ = s.ctx.debug_junction_profile_time(w, combine=False, n=warmup + reps, model=False, scan=False)
            out["timed_repetitions"] = int(ms_a.size)
            for key, ms in (("observed_combined_us", ms_a), ("observed_one_atomic_per_end_us", ms_b), ("model_us", ms_m[warmup:]),
                            ("junction_observed_one_atomic_per_end_us", ms_j[warmup:])):
                kit.put_times(out, key, ms)
            out["whole_call_host_clock_ms"] = kit.host_clock_ms(lambda: s.ctx.orientation_support(w, f, l), reps, warmup)
            out["bytes_streamed"] = 12 * Z + 16 * M  # row + (column, count) per contact; the 16-byte records once (gathers: L2)
            rows.append(out)
            print(json.dumps(out), flush=True)
    s.free_gpu()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg3,cfg3_late")
    ap.add_argument("--windows", default="8,1024")
    ap.add_argument("--levels", default="bin,block")
    ap.add_argument("--moves", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_orientation_support.json"))
    a = ap.parse_args()
    doc = dict(what=("the orientation support's passes on one MI355X: median of %d timed repetitions behind %d warm-ups, hipEvents around each pass "
                     "(the observed pass: zero + kernel; its two forms alternate in four blocks, each behind its own warm-ups) "
                     "(tools/orientation_support_bench.py)" % (a.reps, a.warmup)))
    windows = [int(w) for w in a.windows.split(",") if w]
    levels = [x for x in a.levels.split(",") if x]
    doc["results"] = [r for cfg in a.configs.split(",") if cfg for r in measure(cfg, a.moves, a.reps, a.warmup, windows, levels)]
    ok = all(r["observed_combined_us"] <= r["observed_one_atomic_per_end_us"] for r in doc["results"])
    kit.ship_verdict(doc, ok, bool(kit.shipped_flag("ig_host_orient.inc", "ORIENT_SHIP_COMBINE")))
    kit.write_doc(doc, a.out)


if __name__ == "__main__":
    main()
