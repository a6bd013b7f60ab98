#!/usr/bin/env python3
"""The expected contact map's builds (ig_expected_map, csrc/ig_kernels_emap.cuh) timed at the headline shapes
-> profiles/r12_expected_map.json.

Per config (cfg3 behind a number of batch moves, cfg3_late as it is built), from coo=, at max_side 2048 and 512; per build hipEvents
around zero + the passes + the three mirrors (ig_debug_expected_map_time; the tile forms include the wait for the size of their work
list); median of 20 builds behind warm-ups, the forms alternating in four blocks of 3 warm-ups + 5:
  (a) rows: one thread per position, one atomic per image at every change of pixel -- the yardstick, correct for every input;
  (b) tiles: one workgroup per pixel pair that can hold a cis pair, constant tiles written without an evaluation;
  (c) tiles without the constant shortcut;
  and the whole ``ctx.expected_map`` call on the host clock (it adds the copy of three images to the host).
For the shape with the fewest cis pairs the numpy rule (expected_map.expected_host, with a numpy restatement of the model: its
cost, not its bits, is the subject) is timed once on the host.  The file says from which pixel size on the library ships the tile
form (EMAP_TILE_MIN_BIN in csrc/ig_host_emap.inc, 0: never) and whether the figures support that.

  python tools/expected_map_bench.py [--configs cfg3,cfg3_late] [--out profiles/r12_expected_map.json]
"""
import argparse
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import numpy as np

import _report_bench as kit

FORMS = ("rows", "tiles", "tiles_plain")


def numpy_model_q(p):
    """the Rippe curve and its clamps in numpy (f64): what the rule costs on the host, not the device's bits"""
    amp, slope, d_max, v = float(p["c1"]) * float(p["fact"]), float(p["slope"]), float(p["d_max"]), float(p["v_inter"])

    def q(s):
        s = np.asarray(s, np.float64)
        with np.errstate(all="ignore"):
            y = np.where((s > 0) & (s < d_max), amp * np.power(s, slope), 0.0)
        return np.rint(np.minimum(np.maximum(y, v), 2.0 ** 20) * 2.0 ** 32).astype(np.int64)

    return q


def measure(cfg, moves, reps, warmup, sides):
    from instagraal_amd import expected_map as em

    prob, s = kit.make_sampler(cfg, moves)
    rows = []
    ds, contig, stot, _, _ = s.ctx.debug_tables()
    order = s.ctx.contact_map_order().astype(np.int64)
    position = np.full(ds.size, -1, np.int64)
    position[order] = np.arange(order.size)
    for max_side in sides:
        out = dict(config=cfg, moves_before=moves, sub_fragments=int(prob.n_sub_frags), max_side=max_side)
        ref = None
        for form in FORMS:  # every form returns the same bytes
            s.ctx.debug_expected_map_form(form)
            got = s.ctx.expected_map(max_side)
            if ref is None:
                ref = got
            assert all(np.array_equal(got[k], ref[k]) for k in em.IMAGES) and all(got[k] == ref[k] for k in em.SCALARS[:4]), form
            if form == "tiles":
                out.update(tiles_evaluated=got["tiles_evaluated"], tiles_constant=got["tiles_constant"])
        s.ctx.debug_expected_map_form(0)
        assert int(ref["cis_pairs"].sum()) == 2 * ref["linear_cis_pairs"]
        out.update(n_placed=ref["n_placed"], side=ref["side"], bin=ref["bin"], linear_cis_pairs=ref["linear_cis_pairs"], ring_pairs=ref["ring_pairs_total"])
        # the forms alternate in blocks (other work shares the machine: a drift hits all alike)
        timed = lambda form: lambda n: s.ctx.debug_expected_map_time(max_side, form, n)  # noqa: E731
        for form, ms in zip(FORMS, kit.alternate_blocks([timed(form) for form in FORMS], reps, warmup)):
            t = np.concatenate(ms)
            out["timed_builds"] = int(t.size)
            kit.put_times(out, form + "_ms", t)
        out["whole_call_host_clock_ms"] = kit.host_clock_ms(lambda: s.ctx.expected_map(max_side), 5, warmup)
        out["model_values_per_second_rows"] = round(ref["linear_cis_pairs"] / (1e-3 * out["rows_ms"]), 0) if out["rows_ms"] > 0 else None
        rows.append(out)
    host = dict(config=cfg, linear_cis_pairs=rows[0]["linear_cis_pairs"], inputs=(ds, stot, contig, position), params=dict(prob.params), max_side=min(sides))
    s.free_gpu()
    return rows, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg3,cfg3_late")
    ap.add_argument("--sides", default="2048,512")
    ap.add_argument("--moves", type=int, default=2000, help="batch moves in front of the builds at cfg3 (cfg3_late is measured as built)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="leave the numpy rule's time out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_expected_map.json"))
    a = ap.parse_args()
    from instagraal_amd import expected_map as em

    doc = dict(what=("the expected contact map's builds on one MI355X: median of %d timed builds behind %d warm-ups, hipEvents around each build "
                     "(zero + passes + mirrors; the three forms alternate in four blocks, each behind its own warm-ups) (tools/expected_map_bench.py)"
                     % (a.reps, a.warmup)))
    sides = [int(x) for x in a.sides.split(",") if x]
    doc["results"], hosts = [], []
    for cfg in [c for c in a.configs.split(",") if c]:
        rows, host = measure(cfg, 0 if cfg.endswith("_late") else a.moves, a.reps, a.warmup, sides)
        doc["results"] += rows
        hosts.append(host)
    if not a.no_host:
        h = min(hosts, key=lambda x: x["linear_cis_pairs"])
        ds, stot, contig, position = h["inputs"]
        t0 = time.perf_counter()
        want = em.expected_host(ds, stot, contig, position, h["max_side"], numpy_model_q(h["params"]))
        doc["numpy_rule_on_the_host"] = dict(config=h["config"], max_side=h["max_side"], linear_cis_pairs=want["linear_cis_pairs"],
                                             seconds=round(time.perf_counter() - t0, 2),
                                             note="expected_map.expected_host with a numpy model: the enumeration's cost; the other shapes were not measured on the host")
    min_bin = kit.shipped_flag("ig_host_emap.inc", "EMAP_TILE_MIN_BIN")
    doc["tile_form_shipped_from_bin"] = min_bin if min_bin else "never (the row form ships everywhere)"
    tiles_win = {(r["config"], r["max_side"]): r["tiles_ms"] <= r["rows_ms"] for r in doc["results"]}
    doc["tiles_not_above_rows"] = {"%s@%d" % k: bool(v) for k, v in tiles_win.items()}
    shipped_tiles = {(r["config"], r["max_side"]): bool(min_bin) and r["bin"] >= min_bin and r["bin"] > 1 for r in doc["results"]}
    doc["shipped_form_is_what_the_figures_ask_for"] = all(shipped_tiles[k] == tiles_win[k] for k in tiles_win)
    kit.write_doc(doc, a.out)


if __name__ == "__main__":
    main()
