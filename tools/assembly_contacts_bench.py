#!/usr/bin/env python3
"""The passes of the contacts in genome coordinates (ig_assembly_contacts_build, csrc/ig_kernels_lift.cuh) timed
-> profiles/r10_assembly_contacts.json.

Per config (tiny, small, cfg3, cfg3_late), built from coo=, after a number of batch moves, at both levels; median of the timed
repetitions behind warm-ups, hipEvents around each pass (ig_debug_assembly_contacts_time): count / scan / scatter / the three
sort forms / reduce; how many rows and entries each sort form took; the bytes each pass has to move at least and, from them, the
fraction of the HBM rate (--hbm-gbs, the data-sheet figure unless given) the pass reached.  Three yardsticks on the same machine
in the same process:
  (a) ``np.lexsort`` of the same keys on the host (level "sub": the sort is the feature);
  (b) the device build under the limits (1, 1): every row through the long form (a merge sort in global memory);
  (c) the count and scatter passes with one atomic per contact (ig_debug_assembly_contacts_combine(0)), alternating in blocks with
      the shipped form, which issues one atomic per run of a wave's lanes with the same row.
The checksums of the default build and of (b) must agree.

  python tools/assembly_contacts_bench.py [--configs tiny,small,cfg3,cfg3_late] [--out profiles/r10_assembly_contacts.json]
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


def min_bytes(Z, K, U, n_out, level):
    """what each pass has to move at least: the contacts are 12 bytes each (row; column and count), an entry 8"""
    b = dict(count=12 * Z + 4 * U, scan=16 * U, scatter=12 * Z + 8 * K + 16 * U, sort=16 * K, reduce=(16 * K + 12 * n_out + 16 * U) if level == "bin" else 0)
    b["whole"] = 12 * Z + 8 * K + 8 * K + 8 * K + 16 * U  # read the contacts, write and re-read the entries, write them sorted
    return b


def measure(cfg, moves, reps, warmup, hbm_gbs):
    from instagraal_amd import assembly_contacts as ac
    from instagraal_amd.hip_lib import ASSEMBLY_CONTACTS_PASSES as PASSES

    prob, s = kit.make_sampler(cfg, moves)
    Z, M = int(prob.coo_row.size), int(prob.n_sub_frags)
    order = s.ctx.contact_map_order().astype(np.int64)
    position = ac.positions_of(order, M)
    rows = []
    for level in ac.LEVELS:
        out = dict(config=cfg, moves_before=moves, contacts=Z, sub_fragments=M, level=level)
        s.ctx.debug_assembly_contacts_limits(0, 0)
        # the two forms of the passes over the contacts alternate in blocks (other work shares the machine: a drift hits both alike)
        seen = {}

        def timed(combine):
            def form(n):
                s.ctx.debug_assembly_contacts_combine(combine)
                t, seen["checksum"] = s.ctx.debug_assembly_contacts_time(level, n=n)
                return t, seen["checksum"]
            return form

        ms, one = kit.alternate(timed(True), timed(False), reps, warmup, disagree="the two forms of the passes over the contacts disagree")
        ck = seen["checksum"]  # (of every build so far: they agreed block by block)
        s.ctx.debug_assembly_contacts_combine(True)
        out["count_one_atomic_per_contact_us"] = round(1e3 * float(np.median(one[:, 0])), 2)
        out["scatter_one_atomic_per_contact_us"] = round(1e3 * float(np.median(one[:, 2])), 2)
        out["timed_repetitions"] = int(one.shape[0])
        res = s.ctx.assembly_contacts(level)
        forms = s.ctx.debug_assembly_contacts_forms()
        K, U, n_out = res["entries_kept"], res["n_units"], res["entries_out"]
        lens = np.diff(res["rowptr"])
        out.update(n_units=U, entries_kept=K, entries_out=n_out, entries_unplaced=res["entries_unplaced"], forms=forms,
                   row_length_max_of_the_result=int(lens.max()) if lens.size else 0)
        med = np.median(ms, axis=0)
        for k, name in enumerate(PASSES):
            out[name + "_us"] = round(1e3 * float(med[k]), 2)
            out[name + "_min_us"] = round(1e3 * float(ms[:, k].min()), 2)
        out["all_passes_us"] = round(1e3 * float(np.median(ms.sum(axis=1))), 2)
        b = min_bytes(Z, K, U, n_out, level)
        out["bytes_min"] = b
        sort_us = out["sort_short_us"] + out["sort_lds_us"] + out["sort_long_us"]
        frac = lambda nbytes, us: round(nbytes / (us * 1e-6) / (hbm_gbs * 1e9), 4) if us > 0 else None  # noqa: E731
        out["fraction_of_hbm_rate"] = dict(count=frac(b["count"], out["count_us"]), scatter=frac(b["scatter"], out["scatter_us"]), sort=frac(b["sort"], sort_us),
                                           reduce=frac(b["reduce"], out["reduce_us"]) if level == "bin" else None, whole=frac(b["whole"], out["all_passes_us"]))
        out["build_call_host_clock_ms"] = kit.host_clock_ms(lambda: s.ctx.assembly_contacts(level), max(reps // 4, 2), 0)
        # yardstick (b): every row through the long form
        s.ctx.debug_assembly_contacts_limits(1, 1)
        ms_b, ck_b = s.ctx.debug_assembly_contacts_time(level, n=max(warmup, 1) + max(reps // 4, 2))
        assert ck_b == ck, "the long form and the default build disagree"
        out["all_rows_long_form_us"] = round(1e3 * float(np.median(ms_b[max(warmup, 1):].sum(axis=1))), 2)
        out["all_rows_long_form_sort_us"] = round(1e3 * float(np.median(ms_b[max(warmup, 1):, 3:6].sum(axis=1))), 2)
        s.ctx.debug_assembly_contacts_limits(0, 0)
        # yardstick (a): the host's lexsort of the same keys
        if level == "sub":
            a, c = position[prob.coo_row], position[prob.coo_col]
            kept = (a >= 0) & (c >= 0)
            lo, hi = np.minimum(a, c)[kept], np.maximum(a, c)[kept]
            t0 = time.perf_counter()
            by = np.lexsort((hi, lo))
            out["host_lexsort_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
            col = s.ctx.assembly_contacts_fetch(0, min(n_out, 1 << 20))[0]
            assert np.array_equal(col, hi[by][:col.size])
        s.ctx.assembly_contacts_release()
        rows.append(out)
    s.free_gpu()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="tiny,small,cfg3,cfg3_late")
    ap.add_argument("--moves", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM rate the fractions refer to (GB/s; default: the data sheet's 8 TB/s)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_assembly_contacts.json"))
    a = ap.parse_args()
    doc = dict(what=("the passes of ig_assembly_contacts_build on one MI355X: median of %d timed repetitions behind %d warm-ups, hipEvents around "
                     "each pass (tools/assembly_contacts_bench.py); fractions of an HBM rate of %g GB/s" % (a.reps, a.warmup, a.hbm_gbs)))
    doc["results"] = []
    for cfg in [c for c in a.configs.split(",") if c]:
        doc["results"] += measure(cfg, min(a.moves, 300) if cfg in ("tiny", "small") else a.moves, a.reps, a.warmup, a.hbm_gbs)
        json.dump(doc, open(a.out, "w"), indent=1)  # (config by config: a run cut short leaves what it had)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
