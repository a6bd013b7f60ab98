#!/usr/bin/env python3
"""The passes of the placement support (ig_placement_support, csrc/ig_kernels_place.cuh) timed -> profiles/r13_placement_support.json.

Per shape -- cfg3 behind 2 000 batch moves and cfg3_late --, built from coo=, at w = 64 and w = 1024 (min_hosts = w): median of 20 timed
calls per scan form behind warm-ups, hipEvents around each pass (ig_debug_placement_support_time): records / count / rows / scatter /
the three sort forms / reduce / prefix / scan.  The two forms of the scan (a thread per row: the yardstick; a wave per row:
ig_debug_placement_support_form) and the default (by the row's length, PLACE_WAVE_ENTRIES) alternate in blocks; their checksums must
agree.  The yardstick for the emit is the lift's count and scatter at level "sub" (ig_debug_assembly_contacts_time, one atomic per
contact), timed on the same handle in the same process: they stream the same contacts with one emission per contact instead of two.
The JSON records every median, the ratios of the emit passes to the lift's, the rows on either side of the threshold and whether the
wave form's scan is below the thread form's by more than the spread of the blocks -- no pass has a time target set in advance, and
PLACE_WAVE_ENTRIES changes only on that evidence.

  python tools/placement_support_bench.py [--shapes cfg3,cfg3_late] [--windows 64,1024] [--out profiles/r13_placement_support.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import numpy as np

import _report_bench as kit

SHAPES = dict(cfg3=("cfg3", 2000), cfg3_late=("cfg3_late", 0), small=("small", 300), bigctg=("bigctg", 0))  # (the last two: a dry run of the tool)
FORMS = ("thread", "wave", "default")


def wave_entries():
    """PLACE_WAVE_ENTRIES of the source the library is built from"""
    return kit.shipped_flag("ig_kernels_place.cuh", "PLACE_WAVE_ENTRIES")


def measure(shape, windows, reps, warmup):
    from instagraal_amd.hip_lib import ASSEMBLY_CONTACTS_PASSES as LIFT, PLACEMENT_SUPPORT_PASSES as PASSES

    cfg, moves = SHAPES[shape]
    prob, s = kit.make_sampler(cfg, moves)
    Z = int(prob.coo_row.size)
    blocks = 4
    s.ctx.debug_assembly_contacts_combine(False)  # the yardstick: the lift's passes over the same contacts, one atomic per contact
    ms, _ = s.ctx.debug_assembly_contacts_time("sub", n=warmup + reps)
    lift = np.median(ms[warmup:], axis=0)
    s.ctx.debug_assembly_contacts_combine(True)
    s.ctx.assembly_contacts_release()
    rows = []
    for w in windows:
        out = dict(shape=shape, config=cfg, moves_before=moves, contacts=Z, bins=int(prob.n_frags), window=w, min_hosts=w)
        def timed(form):
            def call(n):
                s.ctx.debug_placement_support_form(form)
                return s.ctx.debug_placement_support_time(w, n=n)
            return call

        ms_by = dict(zip(FORMS, kit.alternate_blocks([timed(f) for f in FORMS], reps, warmup, blocks, "the forms of the scan disagree")))
        s.ctx.debug_placement_support_form("default")
        res = s.ctx.placement_support(w)
        out.update(n_contigs=res["n_contigs"], n_guests=res["n_guests"], entries=res["entries"], forms=s.ctx.debug_placement_support_forms(),
                   with_a_best_site=int((res["best_contig"] >= 0).sum()), timed_calls_per_form=int(sum(len(b) for b in ms_by[FORMS[0]])))
        for form in FORMS:
            m = np.concatenate(ms_by[form])
            med = np.median(m, axis=0)
            out[form] = {p + "_us": round(1e3 * float(med[k]), 2) for k, p in enumerate(PASSES)}
            out[form]["all_passes_us"] = round(1e3 * float(np.median(m.sum(axis=1))), 2)
            scan = [float(np.median(b[:, PASSES.index("scan")])) for b in ms_by[form]]
            out[form]["scan_us_block_medians"] = [round(1e3 * v, 2) for v in scan]
        for p in ("count", "scatter"):
            ref = round(1e3 * float(lift[LIFT.index(p)]), 2)
            out["lift_sub_%s_us" % p] = ref
            out["%s_over_lift" % p] = round(out["thread"][p + "_us"] / ref, 3) if ref > 0 else None
        # the wave form wins only where its slowest block is below the thread form's fastest: beyond the run-to-run spread
        out["wave_scan_below_thread_beyond_spread"] = bool(max(out["wave"]["scan_us_block_medians"]) < min(out["thread"]["scan_us_block_medians"]))
        rows.append(out)
    s.free_gpu()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg3,cfg3_late")
    ap.add_argument("--windows", default="64,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_placement_support.json"))
    a = ap.parse_args()
    doc = dict(what=("the passes of ig_placement_support on one MI355X: median of %d timed calls per scan form behind %d warm-ups, hipEvents around "
                     "each pass (tools/placement_support_bench.py); the lift's count and scatter at level sub on the same handle are the yardstick "
                     "for the emit, the thread form for the scan" % (a.reps, a.warmup)),
               wave_entries_the_library_ships=wave_entries())
    doc["results"] = []
    for shape in [c for c in a.shapes.split(",") if c]:
        doc["results"] += measure(shape, [int(w) for w in a.windows.split(",")], a.reps, a.warmup)
        json.dump(doc, open(a.out, "w"), indent=1)  # (shape by shape: a run cut short leaves what it had)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
