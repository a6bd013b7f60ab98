#!/usr/bin/env python3
"""The balancing's rows from a built map (ig_balance_build_snapshot, csrc/ig_kernels_balsnap.cuh) timed against the build from the
contacts (ig_balance_build_units, ig_balance_build) -> the next free profiles/rNN_balance_snapshot.json.

Part "contacts", per config behind a number of batch moves, at 10 kb bins and at the placed bins:
  * the two builds of the SAME rows as whole calls on the host clock (each ends in the download of the rows: a device synchronise),
    alternating in blocks (other work shares the machine: a drift hits both alike), medians, minima and spread; their rows must agree;
  * the snapshot build pass by pass under hipEvents (ig_debug_balance_snapshot_time); at the placed bins also the build from the
    contacts pass by pass (ig_debug_balance_build_time, level "bin": the same units) -- the library has no timed entry for a caller's
    units, so at 10 kb that route has the whole call only;
  * the whole ``write_zoom_levels(balance=...)`` call by both sources on the host clock, alternating.
Part "pairs": 10^8 seeded pairs at 10 kb as in profiles/r20_pairs_lift.json: the snapshot build of their map pass by pass, the whole
build, and build + iterations.
No threshold is set: the file records the numbers.

  python tools/balance_snapshot_bench.py [--part contacts|pairs|both] [--config cfg3] [--pairs 100000000] [--out FILE]
"""
import argparse
import glob
import json
import os
import re
import shutil
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import numpy as np

import _report_bench as kit

BINSIZE = 10_000


def next_profile():
    taken = [int(m.group(1)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*_*")) for m in [re.match(r"r(\d+)_", os.path.basename(p))] if m]
    mine = glob.glob(os.path.join(ROOT, "profiles", "r*_balance_snapshot.json"))
    return mine[0] if mine else os.path.join(ROOT, "profiles", "r%02d_balance_snapshot.json" % (max(taken, default=0) + 1))


def spread(out, key, ms):
    kit.put_times(out, key, ms)
    out[key.replace("_ms", "_spread")] = round(float((np.max(ms) - np.min(ms)) / max(np.median(ms), 1e-9)), 3)


def host_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def rows_checksum(ctx, r):
    col, count = ctx.balance_fetch(0, int(r["rowptr"][-1]))
    return int(r["rowptr"].sum()) * 31 + int(r["total"].sum()) * 7 + int(col.astype(np.int64).sum()) * 3 + int(count.sum())


def passes_of(names, ms, warmup):
    out = {}
    ms = ms[warmup:].astype(np.float64)
    for k, name in enumerate(names):
        spread(out, name + "_ms", ms[:, k])
    spread(out, "all_passes_ms", ms.sum(axis=1))
    return out


def measure_contacts(cfg, moves, reps, warmup, zoom_reps, resolutions):
    from instagraal_amd import assembly_contacts as ac, zoom_levels as zl
    from instagraal_amd.hip_lib import BALANCE_BUILD_PASSES, BALANCE_SNAPSHOT_PASSES

    prob, s = kit.make_sampler(cfg, moves)
    order, table, _ = s._zoom_frame(False)
    parent = prob.np_sub_frags_2_frags["x"].astype(np.int64)
    bins = ac.units_along(parent[order])
    out = dict(config=cfg, moves_before=moves, contacts=int(prob.coo_row.size), positions=int(order.size), levels=[])
    for name, (unit, U) in (("10kb", zl.units_of_positions(table, BINSIZE)), ("bin", (bins, int(bins[-1]) + 1))):
        snap = s.ctx.assembly_contacts_units(unit, U)  # resident from here on: the snapshot build reads it, the other build does not touch it

        def snapshot_form(n):
            ms, ck = [], 0
            for _ in range(n):
                t, r = host_ms(lambda: s.ctx.balance_build_snapshot(2))
                ms.append(t)
                ck = rows_checksum(s.ctx, r)
            return np.array(ms), ck

        def contacts_form(n):
            ms, ck = [], 0
            for _ in range(n):
                t, r = host_ms(lambda: s.ctx.balance_build_units(unit, U, 2))
                ms.append(t)
                ck = rows_checksum(s.ctx, r)
            return np.array(ms), ck

        a, b = kit.alternate(snapshot_form, contacts_form, reps, warmup, disagree="the two builds disagree")
        built = s.ctx.balance_build_snapshot(2)
        lvl = dict(units=name, n_units=int(U), snapshot_entries=snap["entries_out"], rows_entries=built["entries_out"], kept_observed=built["kept_observed"])
        spread(lvl, "snapshot_build_call_ms", a)
        spread(lvl, "contacts_build_call_ms", b)
        lvl["snapshot_over_contacts"] = round(lvl["snapshot_build_call_ms"] / lvl["contacts_build_call_ms"], 3)
        lvl["snapshot_passes"] = passes_of(BALANCE_SNAPSHOT_PASSES, s.ctx.debug_balance_snapshot_time(warmup + reps), warmup)
        if name == "bin":
            lvl["contacts_passes"] = passes_of(BALANCE_BUILD_PASSES, s.ctx.debug_balance_build_time("bin", 2048, 2, warmup + reps), warmup)
        out["levels"].append(lvl)
        s.ctx.balance_release()
    s.ctx.assembly_contacts_release()
    # the whole write_zoom_levels(balance=...) by both sources
    tmp = tempfile.mkdtemp(prefix="ig_balsnap_bench_")
    try:
        def zoom_form(source):
            def form(n):
                ms, ck = [], 0
                for _ in range(n):
                    shutil.rmtree(os.path.join(tmp, source), ignore_errors=True)
                    t, res = host_ms(lambda: s.write_zoom_levels(os.path.join(tmp, source), resolutions, balance=dict(source=source)))
                    ms.append(t)
                    ck = sum(os.path.getsize(os.path.join(r["folder"], "pixels.tsv")) for r in res)
                return np.array(ms), ck
            return form

        a, b = kit.alternate(zoom_form("snapshot"), zoom_form("contacts"), zoom_reps, 0, blocks=zoom_reps, disagree="the two sources wrote other pixels")
        zoom = dict(resolutions=list(resolutions), calls_per_source=int(a.size))
        spread(zoom, "source_snapshot_call_ms", a)
        spread(zoom, "source_contacts_call_ms", b)
        shutil.rmtree(os.path.join(tmp, "plain"), ignore_errors=True)
        zoom["no_balance_call_ms"] = round(host_ms(lambda: s.write_zoom_levels(os.path.join(tmp, "plain"), resolutions))[0], 2)
        out["write_zoom_levels"] = zoom
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    s.free_gpu()
    return out


def measure_pairs(cfg, moves, n, reps, warmup):
    import pairs_lift_bench as plb
    from instagraal_amd.hip_lib import BALANCE_SNAPSHOT_PASSES

    prob, s = kit.make_sampler(cfg, moves)
    table = s.pairs_begin(reserve_pairs=n)
    c1, p1, c2, p2, strands = plb.seeded_pairs(table, n)
    s.ctx.pairs_lift(c1, p1, c2, p2, strands, outputs=False)
    res = s.ctx.pairs_pixels("binsize", BINSIZE)
    out = dict(config=cfg, moves_before=moves, pairs=n, binsize=BINSIZE, n_units=res["n_units"], snapshot_entries=res["entries_out"], pairs_kept=res["entries_kept"])
    out["pixel_build_host_clock_ms"] = kit.host_clock_ms(lambda: s.ctx.pairs_pixels("binsize", BINSIZE), max(reps // 4, 2), 1)
    built = s.ctx.balance_build_snapshot(2)
    out.update(rows_entries=built["entries_out"], kept_observed=built["kept_observed"], band_observed=built["band_observed"], within_observed=built["within_observed"])
    out["snapshot_passes"] = passes_of(BALANCE_SNAPSHOT_PASSES, s.ctx.debug_balance_snapshot_time(warmup + reps), warmup)
    out["snapshot_build_host_clock_ms"] = kit.host_clock_ms(lambda: s.ctx.balance_build_snapshot(2), reps, warmup)
    bins = s._pairs_bins("binsize", BINSIZE)
    t, w = host_ms(lambda: s._balance_snapshot(bins["contig"]))
    out["build_and_iterations"] = dict(host_clock_ms=round(t, 2), n_iters=w["n_iters"], converged=bool(w["converged"]), masked=int(w["masked"].sum()))
    s.ctx.assembly_contacts_release()
    s.pairs_end()
    s.free_gpu()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="both", choices=("contacts", "pairs", "both"))
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--moves", type=int, default=2000)
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--zoom-reps", type=int, default=2)
    ap.add_argument("--resolutions", default="10000,20000,100000,1000000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = a.out or next_profile()
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc["what"] = ("the balancing's rows from a built map on one MI355X against the build from the contacts: whole calls on the host clock (each ends in a "
                   "download), %d timed repetitions behind %d warm-ups per block in four alternating blocks; passes under hipEvents, %d timed repetitions behind "
                   "%d warm-ups; medians with the minimum and the spread (max - min over the median) (tools/balance_snapshot_bench.py)"
                   % ((a.reps + 3) // 4, a.warmup, a.reps, a.warmup))
    moves = min(a.moves, 300) if a.config in ("tiny", "small") else a.moves
    if a.part in ("contacts", "both"):
        doc["contacts"] = measure_contacts(a.config, moves, a.reps, a.warmup, a.zoom_reps, tuple(int(b) for b in a.resolutions.split(",") if b))
        json.dump(doc, open(out, "w"), indent=1)  # (part by part: a run cut short leaves what it had)
    if a.part in ("pairs", "both"):
        doc["pairs"] = measure_pairs(a.config, moves, a.pairs, a.reps, a.warmup)
    kit.write_doc(doc, out)


if __name__ == "__main__":
    main()
