#!/usr/bin/env python3
"""The fixed-resolution maps (ig_assembly_contacts_build_units, ig_assembly_contacts_coarsen, csrc/ig_kernels_zoom.cuh) timed
-> profiles/r17_zoom_levels.json.

Per config (cfg3, cfg3_late), built from coo=, behind a number of batch moves:
  * the direct build at the finest bin size of the list: the whole call on the host clock;
  * per level of the list whose bin size is a multiple of the one before it (``zoom_levels.plan``): the coarsening from the level
    before against the direct build of the same level, alternating in blocks (other work shares the machine: a drift hits both
    alike), both as whole calls on the host clock -- the table's check and upload, the passes, the rows' download --; the level
    before is rebuilt, untimed, in front of every timed coarsening, and the two results must agree;
  * the passes of a coarsening (ig_debug_zoom_time, hipEvents around each) of the finest level to the next;
  * ``np.unique`` over the same keys on the host: the baseline.
``ship_verdict``: ``zoom_levels.plan`` prefers the coarsening wherever it applies; it is what the figures ask for if at no level the
direct build is faster on every config measured.

  python tools/zoom_levels_bench.py [--configs cfg3,cfg3_late] [--out profiles/r17_zoom_levels.json]
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


def host_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def measure(cfg, moves, resolutions, reps, warmup):
    from instagraal_amd import assembly_contacts as ac, zoom_levels as zl
    from instagraal_amd.hip_lib import ZOOM_PASSES

    prob, s = kit.make_sampler(cfg, moves)
    order, table, _ = s._zoom_frame(False)
    sizes = ac.chrom_sizes(table)
    out = dict(config=cfg, moves_before=moves, contacts=int(prob.coo_row.size), positions=int(order.size), scaffolds=int(sizes[0].size),
               genome_bp=int(sizes[1].sum()), levels=[])
    units = {B: zl.units_of_positions(table, B) for B in resolutions}
    B0 = resolutions[0]
    res = s.ctx.assembly_contacts_units(*units[B0])
    out["finest"] = dict(binsize=B0, n_units=res["n_units"], entries_kept=res["entries_kept"], entries_out=res["entries_out"],
                         units_without_position=zl.units_without_position(*units[B0]),
                         direct_build_host_clock_ms=kit.host_clock_ms(lambda: s.ctx.assembly_contacts_units(*units[B0]), reps, warmup))

    def check(r):
        return int(r["rowptr"].sum()) * 31 + r["entries_out"] * 7 + r["contacts_kept"]

    for i, (B, made) in enumerate(zip(resolutions, zl.plan(resolutions))):
        if made[0] != "coarsen":
            continue
        prev = resolutions[i - 1]
        m, C_ = zl.coarse_map(sizes, prev, made[1])

        def coarsen_form(n):
            ms, ck = [], 0
            for _ in range(n):
                s.ctx.assembly_contacts_units(*units[prev])  # (untimed: the level before, resident)
                t, r = host_ms(lambda: s.ctx.assembly_contacts_coarsen(m, C_))
                ms.append(t)
                ck = check(r)
            return np.array(ms), ck

        def direct_form(n):
            ms, ck = [], 0
            for _ in range(n):
                t, r = host_ms(lambda: s.ctx.assembly_contacts_units(*units[B]))
                ms.append(t)
                ck = check(r)
            return np.array(ms), ck

        a, b = kit.alternate(coarsen_form, direct_form, reps, warmup, disagree="the coarsening and the direct build disagree")
        fine = s.ctx.assembly_contacts_units(*units[prev])
        lvl = dict(binsize=B, from_binsize=prev, factor=made[1], fine_units=fine["n_units"], fine_entries=fine["entries_out"], n_units=C_)
        kit.put_times(lvl, "coarsen_call_ms", a)
        kit.put_times(lvl, "direct_call_ms", b)
        lvl["coarsen_not_slower"] = bool(lvl["coarsen_call_ms"] <= lvl["direct_call_ms"])
        out["levels"].append(lvl)
    # the passes of one coarsening: the finest level to the next of the list that is a multiple of it (else two units to one)
    s.ctx.assembly_contacts_units(*units[B0])
    f = resolutions[1] // B0 if len(resolutions) > 1 and resolutions[1] % B0 == 0 else 2
    m, C_ = zl.coarse_map(sizes, B0, f)
    ms, ck = s.ctx.debug_zoom_time(warmup + reps, m, C_)
    passes = dict(factor=f, forms=None)
    for k, name in enumerate(ZOOM_PASSES):
        kit.put_times(passes, name + "_us", ms[warmup:, k])
    kit.put_times(passes, "all_passes_us", ms[warmup:].sum(axis=1))
    # the baseline: np.unique over the same keys on the host
    fine = s.ctx.assembly_contacts_units(*units[B0])
    col, count = s.ctx.assembly_contacts_fetch(0, fine["n_entries"])
    lo, hi = m[ac.rows_of(fine["rowptr"])], m[col.astype(np.int64)]
    t0 = time.perf_counter()
    keys, inverse = np.unique(lo * C_ + hi, return_inverse=True)
    summed = np.zeros(keys.size, np.int64)
    np.add.at(summed, inverse.ravel(), count)
    passes["host_unique_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
    got = s.ctx.assembly_contacts_coarsen(m, C_)
    passes["forms"] = s.ctx.debug_assembly_contacts_forms()
    g_col, g_count = s.ctx.assembly_contacts_fetch(0, got["n_entries"])
    assert np.array_equal(keys, ac.rows_of(got["rowptr"]) * C_ + g_col) and np.array_equal(summed, g_count), "the device and the host disagree"
    out["passes"] = passes
    s.ctx.assembly_contacts_release()
    s.free_gpu()
    return out


def main():
    from instagraal_amd import zoom_levels as zl

    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg3,cfg3_late")
    ap.add_argument("--moves", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--resolutions", default=",".join(str(b) for b in zl.DEFAULT_RESOLUTIONS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_zoom_levels.json"))
    a = ap.parse_args()
    resolutions = zl.check_resolutions([int(b) for b in a.resolutions.split(",") if b])
    doc = dict(what=("the fixed-resolution maps on one MI355X: whole calls on the host clock, median of %d timed repetitions behind %d warm-ups per block, "
                     "four blocks in which the coarsening and the direct build alternate; the passes of a coarsening under hipEvents "
                     "(tools/zoom_levels_bench.py)" % ((a.reps + 3) // 4, a.warmup)), resolutions=list(resolutions), results=[])
    for cfg in [c for c in a.configs.split(",") if c]:
        doc["results"].append(measure(cfg, min(a.moves, 300) if cfg in ("tiny", "small") else a.moves, resolutions, a.reps, a.warmup))
        json.dump(doc, open(a.out, "w"), indent=1)  # (config by config: a run cut short leaves what it had)
    by_level = {}
    for r in doc["results"]:
        for lvl in r["levels"]:
            by_level.setdefault(lvl["binsize"], []).append(lvl["coarsen_not_slower"])
    doc["ship_verdict"] = dict(direct_faster_on_every_config_at={str(B): not any(v) for B, v in by_level.items()},
                               plan_prefers_the_coarsening_wherever_it_applies=True,
                               shipped_plan_is_what_the_figures_ask_for=all(any(v) for v in by_level.values()))
    kit.write_doc(doc, a.out)


if __name__ == "__main__":
    main()
