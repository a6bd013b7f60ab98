#!/usr/bin/env python3
"""The read pairs lifted onto the current genome (ig_pairs_lift, ig_pairs_pixels_build, ig_pairs_law, csrc/ig_kernels_pairs.cuh) timed
-> the next free profiles/rNN_pairs_lift.json.

On one config (cfg3), built from coo=, behind a number of batch moves, with seeded pairs (80 % on one input contig, every end covered):
  * the three passes and the pixel build at 10 kb under hipEvents (ig_debug_pairs_time): the median of the timed repetitions behind
    the warm-ups, with the minimum and the spread (the largest minus the smallest sample over the median);
  * pairs per second and the bytes k_pairs_lift must move (17 B read per pair, 25 B written per kept pair; the table stays in cache)
    against the measured HBM copy rate;
  * the whole calls on the host clock: the lift of the arrays (upload through the staging arrays included), the pixel build, the law;
  * the vectorised numpy rule (pairs_lift.lift_host, pixels_host, law_host) on the same arrays, chunk by chunk, its pixels and
    histogram compared with the device's;
  * ``--reference-loop N`` (where the reference checkout is, no GPU needed): the reference's own per-line lookups on N pairs of a
    small assembly, extrapolated to the pair count and labelled as such, merged into the newest profile.

  python tools/pairs_lift_bench.py [--config cfg3] [--pairs 100000000] [--out profiles/rNN_pairs_lift.json]
"""
import argparse
import glob
import json
import os
import re
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import numpy as np

import _report_bench as kit

HBM_COPY_BYTES_PER_S = 6.29e12  # the measured copy rate of one MI355X (float4 copy)
BINSIZE = 10_000


def next_profile():
    taken = [int(m.group(1)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*_*")) for m in [re.match(r"r(\d+)_", os.path.basename(p))] if m]
    return os.path.join(ROOT, "profiles", "r%02d_pairs_lift.json" % (max(taken, default=0) + 1))


def seeded_pairs(table, n, seed=0, cis=0.8, piece=10_000_000):
    """n covered pairs as int32 arrays and strand codes: an interval drawn by length and a base inside it per end; the second end on the
    same input contig with probability ``cis``"""
    rng = np.random.default_rng(seed)
    iv, rowptr = table["intervals"], table["src_rowptr"]
    ln = (iv["src_end"] - iv["src_start"]).astype(np.float64)
    cum = np.cumsum(ln) / ln.sum()
    out = [np.zeros(n, np.int32) for _ in range(4)] + [np.zeros(n, np.uint8)]
    for a in range(0, n, piece):
        m = min(piece, n - a)
        i1 = np.minimum(np.searchsorted(cum, rng.random(m)), iv.size - 1)
        c = iv["src_contig"][i1]
        same = rng.random(m) < cis
        i_cis = rowptr[c] + (rng.random(m) * (rowptr[c + 1] - rowptr[c])).astype(np.int64)
        i2 = np.where(same, i_cis, np.minimum(np.searchsorted(cum, rng.random(m)), iv.size - 1))
        for k, i in ((0, i1), (2, i2)):
            out[k][a:a + m] = iv["src_contig"][i]
            out[k + 1][a:a + m] = iv["src_start"][i] + 1 + (rng.random(m) * (iv["src_end"][i] - iv["src_start"][i])).astype(np.int64)
        out[4][a:a + m] = rng.integers(0, 4, m)
    return out


def spread(out, key, ms):
    kit.put_times(out, key, ms)
    out[key.replace("_ms", "_spread")] = round(float((np.max(ms) - np.min(ms)) / max(np.median(ms), 1e-9)), 3)


def measure(cfg, moves, n, reps, warmup, numpy_chunk):
    from instagraal_amd import assembly_contacts as ac, pairs_lift as pl
    from instagraal_amd.hip_lib import PAIRS_PASSES

    prob, s = kit.make_sampler(cfg, moves)
    table = s.pairs_begin(reserve_pairs=n)
    c1, p1, c2, p2, strands = seeded_pairs(table, n)
    edges = pl.default_edges_bp(s.mean_kb(), float(table["scaffold_len"].max()) / 1000.0)
    out = dict(config=cfg, moves_before=moves, pairs=n, intervals=int(table["intervals"].size), scaffolds=int(table["scaffold_len"].size),
               genome_bp=int(table["scaffold_len"].sum()), binsize=BINSIZE, edges=int(edges.size))
    ms, ck = s.ctx.debug_pairs_time(c1, p1, c2, p2, strands, "binsize", BINSIZE, edges, n=warmup + reps)
    ms = ms[warmup:].astype(np.float64)
    passes = {}
    for k, name in enumerate(PAIRS_PASSES):
        spread(passes, name + "_ms", ms[:, k])
    spread(passes, "pixel_build_ms", ms[:, 1:-1].sum(axis=1))
    out["passes"] = passes
    res = s.ctx.pairs_pixels("binsize", BINSIZE)
    kept = res["entries_kept"]
    lift_s = passes["lift_ms"] * 1e-3
    out["lift"] = dict(pairs_kept=kept, pairs_per_second=round(n / lift_s), bytes_moved=17 * n + 25 * kept,
                       bytes_per_second=round((17 * n + 25 * kept) / lift_s), share_of_hbm_copy_rate=round((17 * n + 25 * kept) / lift_s / HBM_COPY_BYTES_PER_S, 4))
    out["pixels"] = dict(n_units=res["n_units"], entries_out=res["entries_out"], forms=s.ctx.debug_assembly_contacts_forms())

    def lift_call():
        s.ctx.pairs_clear()
        s.ctx.pairs_lift(c1, p1, c2, p2, strands, outputs=False)

    host_reps, host_warm = max(reps // 4, 2), 1
    out["host_clock"] = dict(lift_arrays_ms=kit.host_clock_ms(lift_call, host_reps, host_warm),
                             pixel_build_ms=kit.host_clock_ms(lambda: s.ctx.pairs_pixels("binsize", BINSIZE), host_reps, host_warm),
                             law_ms=kit.host_clock_ms(lambda: s.ctx.pairs_law(edges), host_reps, host_warm))
    dev_px = s.ctx.pairs_pixels("binsize", BINSIZE)
    dev_col, dev_count = s.ctx.assembly_contacts_fetch(0, dev_px["n_entries"])
    dev_law = s.ctx.pairs_law(edges)[0]
    # the numpy rule on the same arrays, chunk by chunk; the pixels summed over the chunks by one more unique
    t_lift = t_px = t_law = 0.0
    keys, sums, law = [], [], np.zeros_like(dev_law)
    U = dev_px["n_units"]
    for a in range(0, n, numpy_chunk):
        sl = slice(a, min(a + numpy_chunk, n))
        t0 = time.perf_counter()
        lifted = pl.lift_host(table, c1[sl], p1[sl], c2[sl], p2[sl])
        t1 = time.perf_counter()
        px = pl.pixels_host(lifted, table, BINSIZE)
        t2 = time.perf_counter()
        law += pl.law_host(lifted, strands[sl], edges)
        t3 = time.perf_counter()
        t_lift, t_px, t_law = t_lift + t1 - t0, t_px + t2 - t1, t_law + t3 - t2
        keys.append(ac.rows_of(px["rowptr"]) * U + px["col"])
        sums.append(px["count"])
    t0 = time.perf_counter()
    k_all, inv = np.unique(np.concatenate(keys), return_inverse=True)
    c_all = np.zeros(k_all.size, np.int64)
    np.add.at(c_all, inv.ravel(), np.concatenate(sums))
    t_px += time.perf_counter() - t0
    assert np.array_equal(k_all, ac.rows_of(dev_px["rowptr"]) * U + dev_col) and np.array_equal(c_all, dev_count) and np.array_equal(law, dev_law), "the device and the rule disagree"
    out["numpy_rule"] = dict(chunk=numpy_chunk, lift_ms=round(1e3 * t_lift, 1), pixels_ms=round(1e3 * t_px, 1), law_ms=round(1e3 * t_law, 1), agrees_with_the_device=True)
    out["reference_loop"] = "not timed yet"
    s.ctx.assembly_contacts_release()
    s.pairs_end()
    s.free_gpu()
    return out


def reference_loop(n_lines, extrapolate_to):
    """the reference's own two lookups per line on the golden's assembly (tools/gen_golden_pairs.py), no GPU"""
    import tempfile
    import types

    import gen_golden_pairs as gg
    from instagraal_amd import io_frags, pairs_lift as pl

    post = gg.import_reference_post()
    prob, state = gg.make_state()
    soa, sub = prob.S_o_A_frags, prob.S_o_A_sub_frags
    n_contigs = int(np.max(sub["id_c"]))
    names = {"ctg%d" % c: c for c in range(1, n_contigs + 1)}
    table = pl.table_of_state(state, prob.np_sub_frags_id, prob.np_sub_frags_2_frags["x"].astype(np.int64), sub["id_c"], sub["len_bp"], names=names)
    with tempfile.TemporaryDirectory() as tmp:
        vect = types.SimpleNamespace(id_c=state[2], pos=state[0], ori=state[13], activ=state[15], id_d=state[16])
        start = np.asarray(soa["start_bp"], np.int64)
        end = start + np.asarray(soa["len_bp"], np.int64)
        seqs = {"ctg%d" % c: "A" * int(end[np.asarray(soa["id_c"]) == c].max()) for c in range(1, n_contigs + 1)}
        io_frags.write_assembly(vect, ["ctg%d" % c for c in soa["id_c"]], start.tolist(), end.tolist(), seqs, os.path.join(tmp, "g.fa"), os.path.join(tmp, "info.txt"))
        index = post._build_liftover_index(post._build_new_bins(post.parse_info_frags(os.path.join(tmp, "info.txt")), junction_len=0))
    c1, p1, c2, p2, _ = seeded_pairs(table, n_lines, seed=1)
    name_of = {v: k for k, v in names.items()}
    n1, n2 = [name_of[int(c)] for c in c1], [name_of[int(c)] for c in c2]
    q1, q2 = p1.tolist(), p2.tolist()
    t0 = time.perf_counter()
    for k in range(n_lines):
        post._pos_to_new_coords(n1[k], q1[k], index)
        post._pos_to_new_coords(n2[k], q2[k], index)
    dt = time.perf_counter() - t0
    t0 = time.perf_counter()
    pl.lift_host(table, c1, p1, c2, p2)
    dt_rule = time.perf_counter() - t0
    return dict(lines=n_lines, seconds=round(dt, 3), lines_per_second=round(n_lines / dt), numpy_rule_seconds_on_the_same_lines=round(dt_rule, 4),
                extrapolated_to_pairs=extrapolate_to, extrapolated_seconds=round(dt * extrapolate_to / n_lines, 1),
                note="the two lookups per line only (no parsing, no pixel dictionary), on the CPU this was run on; extrapolated linearly, not measured at that count")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--moves", type=int, default=2000)
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--numpy-chunk", type=int, default=10_000_000)
    ap.add_argument("--reference-loop", type=int, default=0, help="time the reference's per-line lookups on this many lines (no GPU) and merge them into the newest profile")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reference_loop:
        newest = a.out or sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pairs_lift.json")))[-1]
        doc = json.load(open(newest))
        doc["result"]["reference_loop"] = reference_loop(a.reference_loop, doc["result"]["pairs"])
        kit.write_doc(doc, newest, show=doc["result"]["reference_loop"])
        return
    out = a.out or next_profile()
    doc = dict(what=("read pairs lifted onto the current genome on one MI355X: the passes under hipEvents, median of %d timed repetitions behind %d warm-ups, with the "
                     "minimum and the spread (max - min over the median); the whole calls on the host clock; the numpy rule on the same arrays "
                     "(tools/pairs_lift_bench.py)" % (a.reps, a.warmup)))
    doc["result"] = measure(a.config, min(a.moves, 300) if a.config in ("tiny", "small") else a.moves, a.pairs, a.reps, a.warmup, a.numpy_chunk)
    kit.write_doc(doc, out)


if __name__ == "__main__":
    main()
