#!/usr/bin/env python3
"""The cut and join scores (ig_cut_scores, ig_join_scores_build; csrc/ig_kernels_cutjoin.cuh) timed -> the next free
profiles/rNN_cut_join.json.

Per config (cfg3, cfg3_late), built from coo=, behind a number of batch moves:
  * the passes of both reports under hipEvents (the median of the repetitions behind the warm-ups), and the whole calls on the host clock;
  * next to them the same candidates through ``ig_edit_score`` in its default form, as whole calls on the host clock: every cut of the
    longest linear contig, and the four links of each of the 64 pairs with the most contacts;
  * 64 cuts of one contig (the longest) in the delta form against the whole form of ``ig_edit_score``: the shape DESIGN.md 4.23 names as
    the one the delta form loses, every edit of a chunk on ONE contig.
No target is set: the figures go to DESIGN.md 4.24.

  python tools/cut_join_bench.py [--configs cfg3,cfg3_late] [--moves 2000] [--out profiles/rNN_cut_join.json]
"""
import argparse
import glob
import os
import re
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import numpy as np

import _report_bench as kit


def next_free(folder):
    """profiles/rNN_cut_join.json with NN one more than the largest round number a profile carries"""
    rounds = [int(m.group(1)) for m in (re.match(r"r(\d+)", os.path.basename(p)) for p in glob.glob(os.path.join(folder, "r*"))) if m]
    return os.path.join(folder, "r%02d_cut_join.json" % (max(rounds, default=0) + 1))


def clock_ms(fn, reps, warmup):
    t = []
    for _ in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return np.array(t[warmup:])


def measure(cfg, moves, reps, warmup, edit_reps):
    from instagraal_amd import cut_join as cj
    from instagraal_amd.hip_lib import CUT_JOIN_PASSES

    prob, s = kit.make_sampler(cfg, moves)
    state = s.ctx.download_state()
    cuts, joins = s.cut_scores(), s.join_scores()
    out = dict(config=cfg, moves_before=moves, contacts=int(prob.coo_row.size), bins=int(prob.n_frags), sub_fragments=int(prob.n_sub_frags),
               linear_contigs=int(joins["K"]), pairs=int(joins["n_pairs"]), cuts=int(cuts["valid"].sum()), longest_contig_bins=int(state[cj.F["l_cont"]].max()))
    for what in ("cuts", "joins"):
        ms, _ = s.ctx.debug_cut_join_time(what, warmup + reps)
        passes = {}
        for k, p in enumerate(CUT_JOIN_PASSES):
            if ms[warmup:, k].any():
                kit.put_times(passes, p + "_us", ms[warmup:, k])
        out[what + "_passes"] = passes
        kit.put_times(out, what + "_device_ms", ms[warmup:].sum(axis=1))
    kit.put_times(out, "cut_scores_call_ms", clock_ms(s.cut_scores, reps, warmup))
    kit.put_times(out, "join_scores_call_ms", clock_ms(s.join_scores, reps, warmup))
    # the same candidates through the exact scorer
    longest = int(np.argmax(np.where(cuts["valid"], state[cj.F["l_cont"]], 0)))
    bins = np.nonzero(cuts["valid"] & (state[cj.F["id_c"]] == state[cj.F["id_c"]][longest]))[0]
    cut_edits = np.asarray([cj.cut_edit(state, f) for f in bins.tolist()], np.int32).reshape(-1, 5)
    out["exact_cuts_of_the_longest_contig"] = int(cut_edits.shape[0])
    if cut_edits.shape[0]:
        kit.put_times(out, "exact_cuts_call_ms", clock_ms(lambda: s.ctx.edit_score(cut_edits, 0), edit_reps, 1))
        out["exact_cuts_ms_per_cut"] = round(out["exact_cuts_call_ms"] / cut_edits.shape[0], 4)
    rows = cj.link_rows(joins).reshape(-1, 4)
    top = np.argsort(-joins["contacts"], kind="stable")[:64]
    link_edits = np.ascontiguousarray(rows["edit"][top].reshape(-1, 5), np.int32)
    out["exact_links"] = int(link_edits.shape[0])
    if link_edits.shape[0]:
        kit.put_times(out, "exact_links_call_ms", clock_ms(lambda: s.ctx.edit_score(link_edits, 0), edit_reps, 1))
    # 64 cuts of one contig: the delta form against the whole form
    if cut_edits.shape[0] >= 64:
        pick = cut_edits[np.linspace(0, cut_edits.shape[0] - 1, 64).astype(np.int64)]
        one = dict(n_edits=64)
        a, b = kit.alternate(lambda k: (clock_ms(lambda: s.ctx.edit_score(pick, 0), k, 0), 0), lambda k: (clock_ms(lambda: s.ctx.edit_score(pick, 1), k, 0), 0), edit_reps * 4, 1)
        kit.put_times(one, "delta_call_ms", a)
        kit.put_times(one, "whole_call_ms", b)
        one["delta_over_whole"] = round(one["delta_call_ms"] / one["whole_call_ms"], 4)
        assert np.array_equal(s.ctx.edit_score(pick, 0)[1], s.ctx.edit_score(pick, 1)[1]), "the delta form and the whole form disagree"
        out["sixty_four_cuts_of_one_contig"] = one
    s.free_gpu()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg3,cfg3_late")
    ap.add_argument("--moves", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--edit-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = a.out or next_free(os.path.join(ROOT, "profiles"))
    doc = dict(what=("the cut and join scores on one MI355X: the passes under hipEvents, the median (and minimum) of %d repetitions behind %d warm-ups; the whole calls and "
                     "ig_edit_score (default form) on the same candidates on the host clock (each ends in a device synchronise), %d timed calls behind one warm-up; 64 "
                     "cuts of the longest contig in the delta form and the whole form alternating in four blocks (tools/cut_join_bench.py)" % (a.reps, a.warmup, a.edit_reps)),
               results=[])
    for cfg in [c for c in a.configs.split(",") if c]:
        doc["results"].append(measure(cfg, min(a.moves, 300) if cfg in ("tiny", "small") else a.moves, a.reps, a.warmup, a.edit_reps))
        kit.write_doc(doc, out, show={})  # (config by config: a run cut short leaves what it had)
    kit.write_doc(doc, out)


if __name__ == "__main__":
    main()
