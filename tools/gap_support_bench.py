#!/usr/bin/env python3
"""The gap support's passes (ig_gap_support, csrc/ig_kernels_gap.cuh) timed at the headline shapes -> profiles/r16_gap_support.json.

Per config (cfg3, cfg3_late), built from coo=, after a number of batch moves, at block and bin level, at windows of 16 and 256
positions with the 32 default gaps; median of 20 after warm-ups, hipEvents around each pass (ig_debug_gap_support_time; the forms of
the model pass alternate in four blocks of 3 warm-ups + 5):
  (a) the observed pass: one 64-bit atomic per word (the only form that is built);
  (b) the model pass as shipped (a wave per junction of up to GAP_WAVE_TERMS terms, a workgroup beyond);
  (c) the model pass with a wave per junction, (d) with a workgroup per judged junction: equal checksums;
  (e), (f) for orientation k_junc_observed (one atomic per end) and k_junc_model on the same handle at the same window;
  and the whole ``ctx.gap_support`` call on the host clock.
The file records GAP_WAVE_TERMS (a design constant: the results do not depend on it).

  python tools/gap_support_bench.py [--configs cfg3,cfg3_late] [--out profiles/r16_gap_support.json]
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
    from instagraal_amd import gap_support as gs, hip_lib

    prob, s = kit.make_sampler(cfg, moves)
    Z, M = int(prob.coo_row.size), int(prob.n_sub_frags)
    total = int(prob.coo_cnt.astype(np.int64).sum())
    rows = []
    for level in levels:
        for w in windows:
            out = dict(config=cfg, moves_before=moves, contacts=Z, sub_fragments=M, level=level, window=w)
            res = s.gap_support(level=level, window=w)
            j, gaps = res["junction"], res["gaps_kb"]
            out.update(n_junctions=int(j.size), n_gaps=int(gaps.size))
            if j.size == 0:
                rows.append(out)
                print(json.dumps(out), flush=True)
                continue
            assert gs.observed_total(res) == total
            terms = res["pairs"] * int(gaps.size)
            out.update(n_placed=res["n_placed"], n_judged=res["n_judged"], counted_share_of_counts=round(res["counted"] / total, 4),
                       contributions=res["contributions"], atomics_of_the_observed_pass=int(res["contributions"]) * (1 + int(gaps.size)),
                       model_terms=int(terms.sum()), workgroup_junctions=int((terms > hip_lib.GAP_SUPPORT_WAVE_TERMS).sum()),
                       verdicts={v: int((res["verdict"] == v).sum()) for v in ("adjacent", "gap", "apart", "none")})
            # the forms of the model pass alternate in blocks (other work shares the machine: a drift hits all alike)
            forms = ("model", "model_wave", "model_workgroup")
            timed = lambda f: lambda n: s.ctx.debug_gap_support_time(w, j, gaps, which=f, n=n)  # noqa: E731
            ms = dict(zip(forms, kit.alternate_blocks([timed(f) for f in forms], reps, warmup)))
            ms_o, _ = s.ctx.debug_gap_support_time(w, j, gaps, which="observed", n=warmup + reps)
            ms_jo, ms_jm, _, _ = s.ctx.debug_junction_profile_time(w, combine=False, n=warmup + reps, model=True, scan=False)
            out["timed_repetitions"] = int(np.concatenate(ms["model"]).size)
            for key, t in (("observed_us", ms_o[warmup:]), ("model_us", np.concatenate(ms["model"])), ("model_wave_us", np.concatenate(ms["model_wave"])),
                           ("model_workgroup_us", np.concatenate(ms["model_workgroup"])), ("junction_observed_one_atomic_per_end_us", ms_jo[warmup:]),
                           ("junction_model_us", ms_jm[warmup:])):
                kit.put_times(out, key, t)
            out["whole_call_host_clock_ms"] = kit.host_clock_ms(lambda: s.ctx.gap_support(w, j, gaps), reps, warmup)
            out["bytes_streamed"] = 12 * Z + 16 * M  # row + (column, count) per contact; the 16-byte records once (gathers: L2)
            rows.append(out)
            print(json.dumps(out), flush=True)
    s.free_gpu()
    return rows


def main():
    from instagraal_amd import hip_lib

    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg3,cfg3_late")
    ap.add_argument("--windows", default="16,256")
    ap.add_argument("--levels", default="block,bin")
    ap.add_argument("--moves", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_gap_support.json"))
    a = ap.parse_args()
    doc = dict(what=("the gap support's passes on one MI355X: median of %d timed repetitions behind %d warm-ups, hipEvents around each pass (zero + kernel; "
                     "the three forms of the model pass alternate in four blocks, each behind its own warm-ups) (tools/gap_support_bench.py)" % (a.reps, a.warmup)),
               wave_terms=hip_lib.GAP_SUPPORT_WAVE_TERMS, observed_pass_shipped="one_atomic_per_word")
    windows = [int(w) for w in a.windows.split(",") if w]
    levels = [x for x in a.levels.split(",") if x]
    doc["results"] = [r for cfg in a.configs.split(",") if cfg for r in measure(cfg, a.moves, a.reps, a.warmup, windows, levels)]
    kit.write_doc(doc, a.out)


if __name__ == "__main__":
    main()
