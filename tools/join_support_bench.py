#!/usr/bin/env python3
"""The passes of the join support (ig_join_support_build, csrc/ig_kernels_join.cuh) timed -> profiles/r11_join_support.json.

Per shape -- cfg3 behind 2 000 batch moves, cfg3_late, and cfg3 behind ``bomb_the_genome()`` ("bombed_start") --, built from coo=, at
w = 64 and w = 1024: median of the timed builds behind warm-ups, hipEvents around each pass (ig_debug_join_support_time): ends /
count / scan / scatter / the three sort forms / reduce / model.  The two forms of the emit kernel (one atomic per run of a wave's
lanes with the same row, and one atomic per emission: ig_debug_join_support_combine) alternate in blocks; their checksums must
agree.  The yardstick is the lift's count and scatter at level "sub" (ig_debug_assembly_contacts_time), timed on the same handle in
the same process: they stream the same contacts with one emission per contact instead of up to four.  The numpy rule
(join_support.support_host, without the model) is timed on the host.  The JSON records every median, the ratios of the emit passes
to the lift's, and which emit form the library was built with -- no pass has a time target set in advance.

  python tools/join_support_bench.py [--shapes cfg3,cfg3_late,bombed_start] [--windows 64,1024] [--out profiles/r11_join_support.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import numpy as np

import _report_bench as kit

SHAPES = dict(cfg3=("cfg3", 2000, False), cfg3_late=("cfg3_late", 0, False), bombed_start=("cfg3", 0, True),
              small=("small", 300, False), small_bombed=("small", 0, True))  # (the small ones: a dry run of the tool)


def make(cfg, moves, bomb):
    return kit.make_sampler(cfg, moves, prepare=(lambda s: s.bomb_the_genome()) if bomb else None)


def host_inputs(s, prob):
    from instagraal_amd.hip_lib import FRAG_FIELDS

    dist, contig, stot, _, _ = s.ctx.debug_tables()
    state = s.ctx.download_state()
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    order = s.ctx.contact_map_order().astype(np.int64)
    position = np.full(dist.size, -1, np.int64)
    position[order] = np.arange(order.size)
    return dist, stot, contig, position >= 0, position, state[FRAG_FIELDS.index("l_cont_bp")].astype(np.int64)[parent]


def measure(shape, windows, reps, warmup, host):
    from instagraal_amd import join_support as js
    from instagraal_amd.hip_lib import ASSEMBLY_CONTACTS_PASSES as LIFT, JOIN_SUPPORT_PASSES as PASSES

    cfg, moves, bomb = SHAPES[shape]
    prob, s = make(cfg, moves, bomb)
    Z = int(prob.coo_row.size)
    rows = []
    # the yardstick: the lift's passes over the same contacts, one atomic per contact and combined
    lift = {}
    for combine in (False, True):
        s.ctx.debug_assembly_contacts_combine(combine)
        ms, _ = s.ctx.debug_assembly_contacts_time("sub", n=warmup + reps)
        lift[combine] = np.median(ms[warmup:], axis=0)
    s.ctx.debug_assembly_contacts_combine(True)
    s.ctx.assembly_contacts_release()
    t = host_inputs(s, prob) if host else None
    for w in windows:
        out = dict(shape=shape, config=cfg, moves_before=moves, bombed=bomb, contacts=Z, window=w)
        def timed(combine):
            def call(n):
                s.ctx.debug_join_support_combine(combine)
                return s.ctx.debug_join_support_time(w, n=n)
            return call

        ms_by = dict(zip((True, False), kit.alternate(timed(True), timed(False), reps, warmup, disagree="the two forms of the emit kernel disagree")))
        s.ctx.debug_join_support_combine(None)
        res = s.ctx.join_support(w)
        forms = s.ctx.debug_join_support_forms()
        pairs = s.ctx.join_support_fetch(0, res["n_links"])[2]
        s.ctx.join_support_release()
        out.update(n_contigs=res["n_contigs"], n_links=res["n_links"], contributions=res["contributions"], forms=forms,
                   in_reach_observed=res["in_reach_observed"], out_of_reach_observed=res["out_of_reach_observed"],
                   pairs_total=int(pairs.sum()), pairs_max=int(pairs.max()) if pairs.size else 0, timed_builds_per_form=int(ms_by[True].shape[0]))
        for combine, name in ((False, "one_atomic_per_emission"), (True, "combined")):
            m = ms_by[combine]
            med = np.median(m, axis=0)
            out[name] = {p + "_us": round(1e3 * float(med[k]), 2) for k, p in enumerate(PASSES)}
            out[name]["all_passes_us"] = round(1e3 * float(np.median(m.sum(axis=1))), 2)
        for k, p in ((LIFT.index("count"), "count"), (LIFT.index("scatter"), "scatter")):
            out["lift_sub_%s_us" % p] = dict(one_atomic_per_contact=round(1e3 * float(lift[False][k]), 2), combined=round(1e3 * float(lift[True][k]), 2))
            for name in ("one_atomic_per_emission", "combined"):
                ref = out["lift_sub_%s_us" % p]["one_atomic_per_contact" if name.startswith("one") else "combined"]
                out[name]["%s_over_lift" % p] = round(out[name][p + "_us"] / ref, 3) if ref > 0 else None
        out["combined_not_above_yardstick"] = bool(out["combined"]["count_us"] <= out["one_atomic_per_emission"]["count_us"] and
                                                   out["combined"]["scatter_us"] <= out["one_atomic_per_emission"]["scatter_us"])
        if host:
            t0 = time.perf_counter()
            rule = js.support_host(*t, prob.coo_row, prob.coo_col, prob.coo_cnt, w)
            out["host_rule_without_model_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            assert rule["n_links"] == res["n_links"] and np.array_equal(rule["rowptr"], res["rowptr"])
        rows.append(out)
    s.free_gpu()
    return rows


def shipped_form():
    """JOIN_SHIP_COMBINE of the source the library is built from"""
    return "combined" if kit.shipped_flag("ig_host_join.inc", "JOIN_SHIP_COMBINE") else "one_atomic_per_emission"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg3,cfg3_late,bombed_start")
    ap.add_argument("--windows", default="64,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true", help="leave the numpy rule on the host out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_join_support.json"))
    a = ap.parse_args()
    doc = dict(what=("the passes of ig_join_support_build on one MI355X: median of %d timed builds per emit form behind %d warm-ups, hipEvents "
                     "around each pass (tools/join_support_bench.py); the lift's count and scatter at level sub on the same handle are the yardstick"
                     % (a.reps, a.warmup)),
               emit_form_the_library_ships=shipped_form())
    doc["results"] = []
    for shape in [c for c in a.shapes.split(",") if c]:
        doc["results"] += measure(shape, [int(w) for w in a.windows.split(",")], a.reps, a.warmup, not a.no_host)
        json.dump(doc, open(a.out, "w"), indent=1)  # (shape by shape: a run cut short leaves what it had)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
