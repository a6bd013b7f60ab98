#!/usr/bin/env python3
"""The balancing of the contact map (ig_balance_build / ig_balance_run, csrc/ig_kernels_bal.cuh) timed -> profiles/r15_balance.json.

Per shape -- cfg2 and cfg3, built from coo= -- and level -- bin and sub --: the passes of the build (hipEvents around each,
ig_debug_balance_build_time), then, over the built rows, k_bal_marginals alone and one whole iteration (marginals, mean, update,
variance) in each form of the kernel (a wave per row: the yardstick; packed: four short rows per wave), event-timed
(ig_debug_balance_time), the forms alternating in blocks; the whole run to convergence under the default mask per form, by the host's
clock around the call, with the bytes of b, marg_final and variance compared between the forms; and on the host, over the rows fetched
from the device, one iteration of the numpy rule (balance.py: the ordered sum) and one of a plain np.bincount ICE, the baseline.  One
device iteration is checked against the rule's bytes at the size that is timed.  The JSON also states the bytes an iteration must read
-- entries x (column 4 + count 8) + the gathers of b (8 per entry) + the rows and the unit-sized vectors -- and what that makes of the
marginals' time in GB/s.  No time is promised; the default form (BAL_SHIP_FORM) changes only on this evidence.

  python tools/balance_bench.py [--shapes cfg2,cfg3] [--levels bin,sub] [--out profiles/r15_balance.json]
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

FORMS = ("wave", "packed")


def shipped_form():
    return ("default", "wave", "packed")[kit.shipped_flag("ig_host_bal.inc", "BAL_SHIP_FORM")]


def us(ms):
    return round(1e3 * float(np.median(ms)), 2)


def measure(shape, levels, reps, warmup, ignore_diags):
    from instagraal_amd import balance as bal
    from instagraal_amd.hip_lib import BALANCE_BUILD_PASSES as PASSES

    prob, s = kit.make_sampler(shape, 0)
    ctx = s.ctx
    rows = []
    for level in levels:
        out = dict(shape=shape, level=level, contacts=int(prob.coo_row.size), ignore_diags=ignore_diags)
        ms = ctx.debug_balance_build_time(level, 2048, ignore_diags, n=warmup + 5)[warmup:]
        out["build"] = {p + "_us": us(ms[:, k]) for k, p in enumerate(PASSES)}
        out["build"]["all_passes_us"] = us(ms.sum(axis=1))
        ent = ctx.balance_build(level, 2048, ignore_diags)
        U, E = ent["n_units"], ent["entries_out"]
        nnz = ent["nnz"]
        out.update(units=U, entries=E, longest_row=int(nnz.max()), median_row=float(np.median(nnz)), rows_of_at_most_16=int((nnz <= 16).sum()))
        # the bytes one iteration must read: the entries (column, count), the gather of b per entry, the rows; then the vectors of the
        # steps over the units (marg written and read three times, b read twice and written, dd written and read)
        out["marginals_bytes"] = E * (4 + 8) + E * 8 + (U + 1) * 8 + 2 * U * 8
        out["iteration_bytes"] = out["marginals_bytes"] + 8 * U * 8
        blocks = 4
        per = (reps + blocks - 1) // blocks
        by = {(f, w): [] for f in FORMS for w in ("marginals", "iteration")}
        for _ in range(blocks):  # the forms alternate in blocks (other work shares the machine: a drift hits all alike)
            for f in FORMS:
                ctx.debug_balance_form(f)
                for w in ("marginals", "iteration"):
                    by[f, w].append(ctx.debug_balance_time(w, warmup + per)[warmup:])
        masked = bal.mask_units(ent["nnz"], ent["total"])
        b0 = np.where(masked, 0.0, 1.0)
        out["masked_units"] = int(masked.sum())
        runs = {}
        for f in FORMS:
            ctx.debug_balance_form(f)
            res = dict(form=f)
            for w in ("marginals", "iteration"):
                res[w + "_us"] = us(np.concatenate(by[f, w]))
                res[w + "_us_block_medians"] = [us(b) for b in by[f, w]]
            res["marginals_GB_per_s"] = round(out["marginals_bytes"] / (res["marginals_us"] * 1e-6) / 1e9, 1) if res["marginals_us"] > 0 else None
            ctx.balance_run(b0, 1e-5, 200)  # (warm)
            t0 = time.perf_counter()
            runs[f] = ctx.balance_run(b0, 1e-5, 200)
            res["run_to_convergence_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
            res["n_iters"], res["converged"] = runs[f]["n_iters"], runs[f]["converged"]
            out[f] = res
        for k in ("b", "marg_final", "variance"):
            assert np.array_equal(runs["wave"][k].view(np.uint64), runs["packed"][k].view(np.uint64)), "the forms disagree on " + k
        # packed wins only where its slowest block is below the yardstick's fastest: beyond the run-to-run spread
        out["packed_below_wave_beyond_spread"] = bool(max(out["packed"]["marginals_us_block_medians"]) < min(out["wave"]["marginals_us_block_medians"]))
        ctx.debug_balance_form("default")
        one = ctx.balance_run(b0, 0.0, 1)
        col, count = ctx.balance_fetch(0, E)
        ctx.balance_release()
        # the host, over the same rows: one iteration of the rule, one of a plain bincount ICE
        rowptr = ent["rowptr"]
        cf = count.astype(np.float64)
        t0 = time.perf_counter()
        want = bal.iterate(rowptr, col, count, b0, 0.0, 1)
        out["numpy_rule_iteration_and_final_marginals_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        out["device_iteration_equals_the_rule"] = bool(np.array_equal(one["b"].view(np.uint64), want["b"].view(np.uint64))
                                                       and np.array_equal(one["marg_final"].view(np.uint64), want["marg_final"].view(np.uint64))
                                                       and np.array_equal(one["variance"].view(np.uint64), want["variance"].view(np.uint64)))
        assert out["device_iteration_equals_the_rule"], "the device and the rule disagree at the size timed"
        row = np.repeat(np.arange(U), np.diff(rowptr))
        t0 = time.perf_counter()
        marg = np.bincount(row, cf * b0[col], U) * b0
        nz = marg != 0
        m = np.where(nz, marg / marg[nz].mean(), 1.0)
        b1 = b0 / m
        float(((m[nz] - 1.0) ** 2).mean())
        out["numpy_bincount_iteration_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        out["bincount_vs_rule_max_relative_difference"] = float(np.max(np.abs(b1[nz] - want["b"][nz]) / want["b"][nz])) if nz.any() else 0.0
        del col, count, cf, row
        rows.append(out)
    s.free_gpu()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg2,cfg3")
    ap.add_argument("--levels", default="bin,sub")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ignore-diags", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_balance.json"))
    a = ap.parse_args()
    doc = dict(what=("the balancing on one MI355X: the build's passes (median of 5 behind %d warm-ups), k_bal_marginals alone and one whole iteration per "
                     "form (median of %d event-timed launches behind warm-ups, the forms alternating in 4 blocks), the run to convergence by the host's "
                     "clock, and one iteration of the numpy rule and of a plain np.bincount ICE on the host over the same rows "
                     "(tools/balance_bench.py)" % (a.warmup, a.reps)),
               form_the_library_ships=shipped_form())
    doc["results"] = []
    for shape in [c for c in a.shapes.split(",") if c]:
        doc["results"] += measure(shape, [lv for lv in a.levels.split(",") if lv], a.reps, a.warmup, a.ignore_diags)
        json.dump(doc, open(a.out, "w"), indent=1)  # (shape by shape: a run cut short leaves what it had)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
