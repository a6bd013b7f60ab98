#!/usr/bin/env python3
"""The input folder from a FASTA and read pairs (ig_pre_begin, ig_pre_digest, ig_pre_add_pairs, ig_pre_pixels_build,
csrc/ig_kernels_pre.cuh) timed -> the next free profiles/rNN_pre.json.

On a seeded genome (``--bases``, in ``--records`` records, uniform A C G T) under two enzymes (DpnII + HinfI) and ``--pairs`` seeded
pairs (80 % on one record, log-uniform separations):
  * the four passes of the digest and the seven of the pixel build under hipEvents, the assign kernel likewise: the median of the
    timed repetitions behind the warm-ups, with the minimum and the spread (the largest minus the smallest sample over the median);
  * the bytes k_pre_sites must move (every base read once, one bit per base written for the G+C bitmap, the two bitmaps zeroed in
    the same pass) over the time of its pass, against the device-to-device copy rate measured in the same run (a 1 GiB tensor copied:
    read + write);
  * the whole calls on the host clock: the upload, the digest with the fetch of its table, the chunks, the build with its fetch;
  * the numpy rule (pre.digest, pre.gc_counts, pre.pixels_host) on the same arrays, its results compared with the device's;
  * ``--reference-loop N`` (where the reference checkout is, no GPU needed): the reference's own ``_pairs_to_pixels`` on N lines of a
    small genome, extrapolated to the pair count and labelled as such, merged into the newest profile.

  python tools/pre_bench.py [--bases 1000000000] [--pairs 100000000] [--out profiles/rNN_pre.json]
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

ENZYMES = ("DpnII", "HinfI")


def next_profile():
    taken = [int(m.group(1)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*_*")) for m in [re.match(r"r(\d+)_", os.path.basename(p))] if m]
    return os.path.join(ROOT, "profiles", "r%02d_pre.json" % (max(taken, default=0) + 1))


def seeded_genome(n_bases, n_records, seed=0):
    """-> [(name, bytes)]: records of about n_bases / n_records uniform letters (the sizes differ by a few bases, so no record's
    boundary falls on a thread's)"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for k in range(n_records):
        n = n_bases // n_records + 7 * k + 1
        out.append(("ctg%03d" % (k + 1), letters[rng.integers(0, 4, n, dtype=np.uint8)].tobytes()))
    return out


def seeded_pairs(lens, n, seed=1, cis=0.8, piece=10_000_000):
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    cum = np.cumsum(lens) / lens.sum()
    out = [np.zeros(n, np.int32) for _ in range(4)]
    for a in range(0, n, piece):
        m = min(piece, n - a)
        c1 = np.minimum(np.searchsorted(cum, rng.random(m)), lens.size - 1)
        p1 = 1 + (rng.random(m) * lens[c1]).astype(np.int64)
        same = rng.random(m) < cis
        c2 = np.where(same, c1, np.minimum(np.searchsorted(cum, rng.random(m)), lens.size - 1))
        sep = (np.exp(rng.uniform(np.log(50.0), np.log(2.0e6), m)) * rng.choice((-1, 1), m)).astype(np.int64)
        p2 = np.where(same, np.clip(p1 + sep, 1, lens[c1]), 1 + (rng.random(m) * lens[c2]).astype(np.int64))
        for k, v in enumerate((c1, p1, c2, p2)):
            out[k][a:a + m] = v
    return out


def spread(out, key, ms):
    kit.put_times(out, key, ms)
    out[key.replace("_ms", "_spread")] = round(float((np.max(ms) - np.min(ms)) / max(np.median(ms), 1e-9)), 3)


def copy_rate(n_bytes=1 << 30, reps=10):
    """bytes per second of a device-to-device copy (read + write), the median of `reps` behind two warm-ups"""
    import torch

    a = torch.empty(n_bytes, dtype=torch.uint8, device="cuda:0")
    b = torch.empty_like(a)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for r in range(reps + 2):
        ev[0].record()
        b.copy_(a)
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    del a, b
    torch.cuda.empty_cache()
    return 2.0 * n_bytes / (1e-3 * float(np.median(ms[2:])))


def measure(n_bases, n_records, n_pairs, reps, warmup, chunk):
    from instagraal_amd import hip_lib, pre

    records = seeded_genome(n_bases, n_records)
    enzymes = pre.expand_enzymes(list(ENZYMES))
    buf, offs, lens = pre.concatenate(records)
    out = dict(bases=int(lens.sum()), records=n_records, enzymes=list(ENZYMES), pairs=n_pairs, chunk_pairs=chunk)
    rate = copy_rate()
    out["hbm_copy_bytes_per_second_measured"] = round(rate)
    ctx = hip_lib.Context(0)
    t0 = time.perf_counter()
    ctx.pre_begin(buf, offs, lens)
    out["host_clock"] = dict(begin_upload_ms=round(1e3 * (time.perf_counter() - t0), 1))
    ms = np.array([ctx.pre_digest(enzymes, times=True)["ms"] for _ in range(warmup + reps)], np.float64)[warmup:]
    passes = {}
    for k, name in enumerate(hip_lib.PRE_DIGEST_PASSES):
        spread(passes, "digest_" + name + "_ms", ms[:, k])
    spread(passes, "digest_all_ms", ms.sum(axis=1))
    out["host_clock"]["digest_with_fetch_ms"] = kit.host_clock_ms(lambda: ctx.pre_digest(enzymes), max(reps // 4, 2), 1)
    dig = ctx.pre_digest(enzymes)
    out["fragments"] = int(dig["n_frags"])
    sites_s = passes["digest_sites_ms"] * 1e-3
    moved = buf.size + buf.size // 8 + 2 * ((buf.size + 63) // 64) * 8  # the bases read, the G+C bits written, the two bitmaps zeroed
    out["k_pre_sites"] = dict(bytes_moved=int(moved), bytes_per_second=round(moved / sites_s), bases_per_second=round(buf.size / sites_s),
                              share_of_measured_copy_rate=round(moved / sites_s / rate, 4))
    c1, p1, c2, p2 = seeded_pairs(lens, n_pairs)
    assign, build = [], []
    for r in range(warmup + reps):
        ctx.pre_clear()
        t = 0.0
        for a in range(0, n_pairs, chunk):
            t += ctx.pre_add_pairs(c1[a:a + chunk], p1[a:a + chunk], c2[a:a + chunk], p2[a:a + chunk], times=True)["ms"]
        assign.append(t)
    for r in range(warmup + reps):  # the build alone, over the store the last repetition left
        npx, sc, t = hip_lib.C.c_int64(), np.zeros(8, np.int64), np.zeros(len(hip_lib.ASSEMBLY_CONTACTS_PASSES), np.float32)
        hip_lib._ck(hip_lib.lib().ig_pre_pixels_build(ctx._h, hip_lib.C.byref(npx), hip_lib._p(sc), hip_lib._p(t)))
        build.append(t.astype(np.float64))
    spread(passes, "assign_ms", np.array(assign[warmup:]))
    build = np.array(build[warmup:])
    for k, name in enumerate(hip_lib.ASSEMBLY_CONTACTS_PASSES):
        spread(passes, "pixels_" + name + "_ms", build[:, k])
    spread(passes, "pixels_all_ms", build.sum(axis=1))
    out["passes"] = passes
    out["assign"] = dict(pairs_per_second=round(n_pairs / (passes["assign_ms"] * 1e-3)))

    def chunks_call():
        ctx.pre_clear()
        for a in range(0, n_pairs, chunk):
            ctx.pre_add_pairs(c1[a:a + chunk], p1[a:a + chunk], c2[a:a + chunk], p2[a:a + chunk])

    out["host_clock"]["add_pairs_all_chunks_ms"] = kit.host_clock_ms(chunks_call, 2, 1)
    out["host_clock"]["pixels_build_with_fetch_ms"] = kit.host_clock_ms(ctx.pre_pixels, 2, 1)
    px = ctx.pre_pixels()
    out["pixels"] = {k: int(px[k]) for k in pre.SCALARS}
    # the numpy rule on the same arrays
    t0 = time.perf_counter()
    want = pre.digest(records, enzymes)
    t1 = time.perf_counter()
    gc = pre.gc_counts(records, want)
    t2 = time.perf_counter()
    parts = [pre.pixels_host(want, c1[a:a + chunk], p1[a:a + chunk], c2[a:a + chunk], p2[a:a + chunk]) for a in range(0, n_pairs, chunk)]
    host = pre.merge_pixels(parts, want["n_frags"])
    t3 = time.perf_counter()
    ok = all(np.array_equal(dig[k], want[k]) for k in ("rec_first", "frag_rec", "start", "end")) and np.array_equal(dig["gc_count"], gc)
    ok = ok and all(np.array_equal(px[k], host[k]) for k in ("rowptr", "col", "count")) and all(px[k] == host[k] for k in pre.SCALARS)
    assert ok, "the device and the rule disagree"
    out["numpy_rule"] = dict(digest_ms=round(1e3 * (t1 - t0), 1), gc_ms=round(1e3 * (t2 - t1), 1), pixels_ms=round(1e3 * (t3 - t2), 1), agrees_with_the_device=True)
    out["reference_loop"] = "not timed yet"
    ctx.pre_end()
    ctx.close()
    return out


def reference_loop(n_lines, extrapolate_to):
    """the reference's own _pairs_to_pixels on n_lines lines over the golden's genome (tools/gen_golden_pre.py), no GPU"""
    import tempfile

    import pandas as pd

    import gen_golden_pre as gg
    from instagraal_amd import pre

    ref = gg.import_reference_pre()
    records = gg.make_genome(np.random.default_rng(gg.SEED))
    dig = pre.digest(records, list(gg.ENZYMES))
    names = [n for n, _ in records]
    bins = pd.DataFrame({"chrom": [names[r] for r in dig["frag_rec"]], "start": dig["start"], "end": dig["end"]})
    c1, p1, c2, p2 = seeded_pairs(dig["rec_len"], n_lines, seed=2)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in.pairs")
        with open(path, "w") as f:
            f.write("".join("r%d\t%s\t%d\t%s\t%d\t+\t-\n" % (k, names[c1[k]], p1[k], names[c2[k]], p2[k]) for k in range(n_lines)))
        t0 = time.perf_counter()
        pixels, total = ref._pairs_to_pixels(__import__("pathlib").Path(path), bins)
        dt = time.perf_counter() - t0
    t0 = time.perf_counter()
    host = pre.pixels_host(dig, c1, p1, c2, p2)
    dt_rule = time.perf_counter() - t0
    assert host["pairs_kept"] == total and host["pixels"] == len(pixels)
    return dict(lines=n_lines, seconds=round(dt, 3), lines_per_second=round(n_lines / dt), numpy_rule_seconds_on_the_same_pairs=round(dt_rule, 4),
                extrapolated_to_pairs=extrapolate_to, extrapolated_seconds=round(dt * extrapolate_to / n_lines, 1),
                note="the reference's loop with its parsing and its dictionary of pixels, a genome of %d fragments, on the CPU this was run on; extrapolated linearly, not "
                     "measured at that count" % dig["n_frags"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=1_000_000_000)
    ap.add_argument("--records", type=int, default=24)
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--chunk", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reference-loop", type=int, default=0, help="time the reference's pixel loop on this many lines (no GPU) and merge it into the newest profile")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reference_loop:
        newest = a.out or sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pre.json")))[-1]
        doc = json.load(open(newest))
        doc["result"]["reference_loop"] = reference_loop(a.reference_loop, doc["result"]["pairs"])
        kit.write_doc(doc, newest, show=doc["result"]["reference_loop"])
        return
    out = a.out or next_profile()
    doc = dict(what=("the input folder from a FASTA and read pairs on one MI355X: the passes under hipEvents, median of %d timed repetitions behind %d warm-ups, with the "
                     "minimum and the spread (max - min over the median); the whole calls on the host clock; the numpy rule on the same arrays "
                     "(tools/pre_bench.py)" % (a.reps, a.warmup)))
    doc["result"] = measure(a.bases, a.records, a.pairs, a.reps, a.warmup, a.chunk)
    kit.write_doc(doc, out)


if __name__ == "__main__":
    main()
