#!/usr/bin/env python3
"""The contact levels of the pyramid (ig_pyr_begin, ig_pyr_matrix, ig_pyr_degrees, ig_pyr_remap, csrc/ig_kernels_pyr.cuh) timed -> the
next free profiles/rNN_pyramid.json.  Not part of bench.py.

  * The chain: a seeded canonical level 0 of ``--entries`` entries over ``--frags`` fragments (the size of profiles/r21_pre.json's
    pixels: what ``pre`` hands over), the filter's table (1 % of the fragments destroyed, 2 % glued to the next), then ``--levels`` - 1
    binnings by ``--factor``.  Per level: the device's seven passes of the row builder under hipEvents and the whole call on the host
    clock (median of ``--reps`` chains behind one warm-up; every chain uploads the list again), and the host rule
    ``pyramid._accumulate_contacts`` on the same arrays, once.  The two agree, level by level.
  * The whole ``build_and_filter`` call through ``pyramid`` and through ``pyramid_device`` on a folder of ``--whole-frags`` fragments
    (``synth.write_text_dataset_large``), in a memory-backed directory, the device path split into read, tables, device and write; the
    two folders are compared file by file.

  python tools/pyramid_bench.py [--entries 100000000] [--frags 7800000] [--whole-frags 85000] [--dir /dev/shm] [--out profiles/rNN_pyramid.json]
"""
import argparse
import filecmp
import glob
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


def next_profile():
    taken = [int(m.group(1)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*_*")) for m in [re.match(r"r(\d+)_", os.path.basename(p))] if m]
    return os.path.join(ROOT, "profiles", "r%02d_pyramid.json" % (max(taken, default=0) + 1))


def seeded_level0(n_entries, n_frags, seed=5):
    """a canonical list: a uniform, b - a log-uniform (most pixels near the diagonal, as a contact map's), counts 1 .. 40"""
    rng = np.random.default_rng(seed)
    draw = int(n_entries * 1.06)
    a = rng.integers(0, n_frags, draw, dtype=np.int64)
    off = np.exp(rng.uniform(0.0, np.log(n_frags / 4.0), draw)).astype(np.int64)
    b = np.minimum(a + off, n_frags - 1)
    key = np.unique(a * n_frags + b)
    if key.size > n_entries:
        key = key[rng.random(key.size) < n_entries / key.size]
    a, b = key // n_frags, key % n_frags
    return a, b, rng.integers(1, 41, key.size, dtype=np.int64)


def tables(n_frags, levels, factor, seed=6):
    """[(lut, n_new, skip_first)]: the filter's table, then the binnings"""
    rng = np.random.default_rng(seed)
    u = rng.random(n_frags)
    emitted = u >= 0.03  # 1 % destroyed, 2 % glued to the next emitted fragment
    lut = np.cumsum(emitted) - emitted
    n_new = int(emitted.sum())
    lut[lut >= n_new] = -1
    lut[u < 0.01] = -1
    out = [(lut.astype(np.int64), n_new, False)]
    n = n_new
    for _ in range(levels - 1):
        out.append((np.arange(n, dtype=np.int64) // factor, (n + factor - 1) // factor, True))
        n = out[-1][1]
    return out


def chain(n_entries, n_frags, levels, factor, reps):
    from instagraal_amd import hip_lib, pyramid
    from instagraal_amd import pyramid_levels as rule

    a, b, count = seeded_level0(n_entries, n_frags)
    steps = tables(n_frags, levels, factor)
    print("seeded: %d entries" % a.size, file=sys.stderr, flush=True)
    out = dict(entries=int(a.size), fragments=n_frags, levels=levels, factor=factor)
    ctx = hip_lib.Context(0)
    per, clock, upload, fetched = [], [], [], None
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        flag = ctx.pyr_begin(n_frags, a, b, count)
        upload.append(time.perf_counter() - t0)
        assert flag, "the seeded list is canonical"
        ms, dt, sizes, keep = [], [], [], []
        t0 = time.perf_counter()
        sizes.append(ctx.pyr_matrix(times=ms))
        dt.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        deg = ctx.pyr_degrees()
        t_deg = time.perf_counter() - t0
        for lut, n_new, skip in steps:
            t0 = time.perf_counter()
            sc = ctx.pyr_remap(lut, n_new, skip, times=ms)
            dt.append(time.perf_counter() - t0)
            sizes.append(sc["pixels"])
            if rep == 0:  # the warm-up fetches every level: what the rule is held against, and what a build writes
                t0 = time.perf_counter()
                keep.append((ctx.pyr_level()[0], time.perf_counter() - t0))
        ctx.pyr_end()
        print("chain %d: %s pixels" % (rep, sizes), file=sys.stderr, flush=True)
        if rep == 0:
            fetched, deg0 = keep, deg
        else:
            per.append(np.array(ms)), clock.append(dt + [t_deg])
    ctx.close()
    per, clock = np.array(per), np.array(clock)  # [reps][levels + 1][7], [reps][levels + 2]
    out["upload_host_clock_ms"] = round(1e3 * float(np.median(upload[1:])), 1)
    out["degrees_host_clock_ms"] = round(1e3 * float(np.median(clock[:, -1])), 2)
    # the host rule on the same arrays, once per level, and the two agree
    rows = []
    cur = (a, b, count)
    t0 = time.perf_counter()
    f1, f2, tot = pyramid._accumulate_contacts(*cur)
    host_s = time.perf_counter() - t0
    assert np.array_equal(f1, a) and np.array_equal(tot, count) and np.array_equal(deg0, rule.degrees((f1, f2, tot), n_frags)), "the degrees disagree"
    names = ["list -> its level"] + ["filter -> level 0"] + ["level %d -> level %d" % (k, k + 1) for k in range(levels - 1)]
    for k, name in enumerate(names):
        if k > 0:
            lut, n_new, skip = steps[k - 1]
            x, y, c = (v[1:] for v in cur) if skip else cur
            t0 = time.perf_counter()
            nx, ny = lut[x], lut[y]
            ok = (nx >= 0) & (ny >= 0)
            f1, f2, tot = pyramid._accumulate_contacts(nx[ok], ny[ok], c[ok])
            host_s = time.perf_counter() - t0
            d3, fetch_s = fetched[k - 1]
            assert np.array_equal(d3[0], f1) and np.array_equal(d3[1], f2) and np.array_equal(d3[2], tot), "level %d: the device and the host rule disagree" % k
            cur = (f1, f2, tot)
        row = dict(step=name, entries_in=int(a.size if k == 0 else rows[-1]["pixels_out"]), pixels_out=int(f1.size))
        kit.put_times(row, "device_passes_ms", per[:, k, :].sum(axis=1))
        row["device_passes_median_ms"] = {p: round(float(np.median(per[:, k, i])), 4) for i, p in enumerate(hip_lib.ASSEMBLY_CONTACTS_PASSES)}
        row["device_call_host_clock_ms"] = round(1e3 * float(np.median(clock[:, k])), 2)
        if k > 0:
            row["fetch_three_rows_host_clock_ms"] = round(1e3 * fetch_s, 1)
        row["host_rule_accumulate_ms"] = round(1e3 * host_s, 1)
        print("host rule, %s: %.1f s" % (name, host_s), file=sys.stderr, flush=True)
        rows.append(row)
    out["per_level"] = rows
    out["agrees_with_the_host_rule"] = True
    return out


def whole(n_frags, directory):
    from instagraal_amd import pyramid, pyramid_device, synth

    tmp = tempfile.mkdtemp(prefix="pyramid_bench_", dir=directory)
    try:
        data = os.path.join(tmp, "data")
        nf, n_lines = synth.write_text_dataset_large(data, n_frags0=n_frags)
        out = dict(fragments=int(nf), contact_lines=int(n_lines), size_pyramid=9, factor=3)
        t0 = time.perf_counter()
        pyramid.build_and_filter(data, 9, 3, output_folder=os.path.join(tmp, "host")).close()
        out["host"] = dict(seconds=round(time.perf_counter() - t0, 2))
        ch = pyramid_device.Chain(True)
        t0 = time.perf_counter()
        pyramid_device.build_and_filter(data, 9, 3, output_folder=os.path.join(tmp, "dev"), device=True, _chain=ch).close()
        ch.close()
        total = time.perf_counter() - t0
        out["device"] = dict(seconds=round(total, 2), read_s=round(ch.seconds["read"], 2), tables_s=round(ch.seconds["tables"], 2), device_s=round(ch.seconds["device"], 2),
                             write_s=round(ch.seconds["write"], 2), other_s=round(total - sum(ch.seconds.values()), 2),
                             note="device_s: the uploads, the kernels and the fetched levels on the host clock; other_s: the context made, the stores and the loader")
        n = 0
        for base, _, files in os.walk(os.path.join(tmp, "host", "pyramids")):
            for f in files:
                if f.endswith(".txt"):
                    rel = os.path.relpath(os.path.join(base, f), os.path.join(tmp, "host"))
                    assert filecmp.cmp(os.path.join(base, f), os.path.join(tmp, "dev", rel), shallow=False), rel
                    n += 1
        out["text_files_identical"] = n
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--frags", type=int, default=7_800_000)
    ap.add_argument("--levels", type=int, default=9)
    ap.add_argument("--factor", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--whole-frags", type=int, default=85_000)
    ap.add_argument("--dir", default="/dev/shm", help="a memory-backed directory for the whole calls")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    doc = dict(what=("the contact levels of the pyramid on one MI355X: the row builder's passes under hipEvents and the calls on the host clock, median of %d chains behind one "
                     "warm-up; the host rule pyramid._accumulate_contacts on the same arrays, once; the whole build_and_filter call through both paths in a memory-backed "
                     "directory (tools/pyramid_bench.py)" % a.reps))
    doc["chain"] = chain(a.entries, a.frags, a.levels, a.factor, a.reps)
    doc["build_and_filter"] = whole(a.whole_frags, a.dir)
    kit.write_doc(doc, a.out or next_profile())


if __name__ == "__main__":
    main()
