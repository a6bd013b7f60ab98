#!/usr/bin/env python3
"""The segment edits (ig_edit_score, csrc/ig_kernels_edit.cuh) timed -> the next free profiles/rNN_rearrange.json.

Per config (cfg3, cfg3_late), built from coo=, behind a number of batch moves, for lists of 64 and 512 seeded edits over the blocks of
the genome (a block in place and flipped, made a contig of its own, or next to the end of another block):
  * the delta form against the whole form, alternating in blocks (other work shares the machine: a drift hits both alike), as whole
    calls on the host clock, 24 timed calls per form by default, with their 10th and 90th percentile next to the median; the limbs
    of the two forms must agree;
  * the passes of either form under hipEvents (plan, state, tables, delta, zero / whole), summed over the chunks;
  * ``delta_over_whole``: the ratio of the two medians -- what DESIGN.md 4.23 asks for before ``form = 0`` picks a form by shape.

  python tools/rearrange_bench.py [--configs cfg3,cfg3_late] [--sizes 64,512] [--out profiles/rNN_rearrange.json]
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
    """profiles/rNN_rearrange.json with NN one more than the largest round number a profile carries"""
    rounds = [int(m.group(1)) for m in (re.match(r"r(\d+)", os.path.basename(p)) for p in glob.glob(os.path.join(folder, "r*"))) if m]
    return os.path.join(folder, "r%02d_rearrange.json" % (max(rounds, default=0) + 1))


def block_edits(s, n, seed=1):
    """n seeded edits over the blocks of the current genome, every one valid on it"""
    from instagraal_amd import orientation_support as osup, rearrange as ra

    order = s.ctx.contact_map_order().astype(np.int64)
    parent = s.np_sub_frags_2_frags["x"].astype(np.int64)
    g = s.gpu_vect_frags.copy_from_gpu()
    blocks = osup.block_segments(order, parent, g.id_c, g.ori, g.id_d, s.np_init_id_c, s.np_init_pos)
    state = g.soa17()
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        k = int(rng.integers(blocks["first_bin"].size))
        kind = int(rng.integers(4))
        anchor = ra.IN_PLACE if kind == 0 else ra.NEW_CONTIG if kind == 1 else int(blocks["last_bin"][int(rng.integers(blocks["last_bin"].size))])
        e = (int(blocks["first_bin"][k]), int(blocks["last_bin"][k]), anchor, int(rng.integers(2)), int(rng.integers(2)) if kind else 1)
        if ra.check(state, e) == 0:
            out.append(e)
    return np.asarray(out, np.int32)


def measure(cfg, moves, sizes, reps, warmup):
    from instagraal_amd.hip_lib import EDIT_PASSES

    prob, s = kit.make_sampler(cfg, moves)
    g = s.gpu_vect_frags.copy_from_gpu()
    out = dict(config=cfg, moves_before=moves, contacts=int(prob.coo_row.size), bins=int(prob.n_frags), sub_fragments=int(prob.n_sub_frags),
               contigs=int(np.unique(g.id_c).size), longest_contig_bins=int(g.l_cont.max()), lists=[])
    for n in sizes:
        edits = block_edits(s, n)

        def form(which):
            def run(k):
                ms, ck = [], 0
                for _ in range(k):
                    t0 = time.perf_counter()
                    _, limbs, _, _ = s.ctx.edit_score(edits, which)
                    ms.append(1e3 * (time.perf_counter() - t0))
                    ck = int(limbs.sum())
                return np.array(ms), ck
            return run

        a, b = kit.alternate(form(0), form(1), reps, warmup, disagree="the delta form and the whole form disagree")
        row = dict(n_edits=int(n), chunks=(int(n) + 63) // 64)
        kit.put_times(row, "delta_call_ms", a)
        kit.put_times(row, "whole_call_ms", b)
        for key, ms in (("delta", a), ("whole", b)):  # the spread of the timed calls: 10th and 90th percentile, and how many there were
            row[key + "_call_p10_p90_ms"] = [round(float(np.percentile(ms, q)), 4) for q in (10, 90)]
        row["timed_calls_per_form"] = int(a.size)
        row["delta_over_whole"] = round(row["delta_call_ms"] / row["whole_call_ms"], 4)
        row["delta_not_slower"] = bool(row["delta_call_ms"] <= row["whole_call_ms"])
        for which, name in ((0, "delta_form"), (1, "whole_form")):
            ms, _ = s.ctx.debug_edit_time(edits, which, warmup + reps)
            passes = {}
            for k, p in enumerate(EDIT_PASSES):
                kit.put_times(passes, p + "_us", ms[warmup:, k])
            row[name + "_passes"] = passes
        out["lists"].append(row)
    s.free_gpu()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg3,cfg3_late")
    ap.add_argument("--moves", type=int, default=2000)
    ap.add_argument("--sizes", default="64,512")
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = a.out or next_free(os.path.join(ROOT, "profiles"))
    sizes = [int(x) for x in a.sizes.split(",") if x]
    doc = dict(what=("the segment edits on one MI355X: ig_edit_score as whole calls on the host clock (each ends in a device synchronise), the delta form "
                     "and the whole form alternating in four blocks of %d timed calls behind %d warm-up(s) each; per form the median, the minimum and the "
                     "10th / 90th percentile over all its timed calls; the passes under hipEvents, the median of %d repetitions behind %d warm-up(s), "
                     "summed over the chunks (tools/rearrange_bench.py)" % ((a.reps + 3) // 4, a.warmup, a.reps, a.warmup)), sizes=sizes, results=[])
    for cfg in [c for c in a.configs.split(",") if c]:
        doc["results"].append(measure(cfg, min(a.moves, 300) if cfg in ("tiny", "small") else a.moves, sizes, a.reps, a.warmup))
        kit.write_doc(doc, out, show={})  # (config by config: a run cut short leaves what it had)
    rows = [r for res in doc["results"] for r in res["lists"]]
    doc["ship_verdict"] = dict(delta_form_not_slower_everywhere=all(r["delta_not_slower"] for r in rows), form_0_is="delta",
                               shipped_form_is_what_the_figures_ask_for=all(r["delta_not_slower"] for r in rows))
    kit.write_doc(doc, out)


if __name__ == "__main__":
    main()
