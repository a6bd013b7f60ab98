#!/usr/bin/env python3
"""The polished FASTA of the polish step (ig_seq_begin, ig_seq_composition, ig_seq_plan, ig_seq_window, csrc/ig_kernels_seq.cuh) timed
-> the next free profiles/rNN_polish.json.  Not part of bench.py.

On a seeded genome (``--bases`` in ``--records`` records, uniform A C G T) and an info_frags of about ``--bins`` bins: every scaffold
holds one block of every record, 30 % of the blocks reversed, a few bins left out (the lost DNA):
  * k_seq_stitch per window and summed over the file, under hipEvents: the median of the timed walks behind the warm-ups with the
    minimum and the spread (max - min over the median); once for walks that count the classes of the bases as they stitch (the first walk
    behind a plan) and once for walks that only stitch -- the difference is what the counting costs in the kernel;
  * the composition pass over the input likewise;
  * the device-to-device copy rate measured in the same run (a 1 GiB tensor copied: read + write), and the kernel's bytes (every file
    byte written, every base read once) per second against it;
  * the whole ``polish_assembly`` call with the device and with ``device=False``, the file written to a memory-backed directory, with
    the seconds of its parts: reading the FASTA, the list work, the stitching (upload, kernels, download, writing).

  python tools/polish_bench.py [--bases 1000000000] [--bins 200000] [--dir /dev/shm] [--out profiles/rNN_polish.json]
"""
import argparse
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
from pre_bench import copy_rate, seeded_genome, spread


def next_profile():
    taken = [int(m.group(1)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*_*")) for m in [re.match(r"r(\d+)_", os.path.basename(p))] if m]
    return os.path.join(ROOT, "profiles", "r%02d_polish.json" % (max(taken, default=0) + 1))


def seeded_scaffolds(records, n_bins, reversed_share=0.3, left_out=0.002, seed=3):
    """one scaffold per record index s: the block s + r (mod R) of every record r, a block reversed as a whole with ``reversed_share``"""
    rng = np.random.default_rng(seed)
    R = len(records)
    per = max(n_bins // R, R)
    blocks = []
    for r, (name, seq) in enumerate(records):
        cuts = np.linspace(0, len(seq), per + 1).astype(np.int64)
        bins = [[name, k, int(cuts[k]), int(cuts[k + 1]), 1] for k in range(per) if rng.random() >= left_out]
        size = -(-len(bins) // R)
        blocks.append([bins[a:a + size] for a in range(0, len(bins), size)])
    scaffolds = {}
    for s in range(R):
        out = []
        for r in range(R):
            blk = blocks[r][(s + r) % R] if (s + r) % R < len(blocks[r]) else []
            out += [b[:4] + [-1] for b in reversed(blk)] if rng.random() < reversed_share else blk
        scaffolds["scaffold%02d" % s] = out
    return scaffolds


def measure(n_bases, n_records, n_bins, reps, warmup, window, directory):
    from instagraal_amd import hip_lib, pre
    from instagraal_amd import scaffold_polish as sp

    records = seeded_genome(n_bases, n_records)
    scaffolds = seeded_scaffolds(records, n_bins)
    plan = sp.stitch_plan(records, scaffolds)
    buf, offs, lens = pre.concatenate(records)
    n_pieces = int(plan["src"].size)
    out = dict(bases=int(lens.sum()), records=n_records, bins=sum(len(s) for s in scaffolds.values()), pieces=n_pieces, pieces_reversed=int((plan["ori"] < 0).sum()),
               file_bytes=plan["file_bytes"], window_bytes=window, width=plan["width"])
    rate = copy_rate()
    out["hbm_copy_bytes_per_second_measured"] = round(rate)
    ctx = hip_lib.Context(0)
    t0 = time.perf_counter()
    ctx.seq_begin(buf, offs, lens)
    out["host_clock"] = dict(begin_upload_ms=round(1e3 * (time.perf_counter() - t0), 1))
    passes = {}
    times = {}
    for _ in range(warmup + reps):
        comp = ctx.seq_composition(times=times)
    spread(passes, "composition_ms", np.array(times["composition"][warmup:]))
    view = np.empty(min(window, plan["file_bytes"]), np.uint8)
    firsts = list(range(0, plan["file_bytes"], window))

    def walk(keep=None):
        t = {}
        t0 = time.perf_counter()
        for first in firsts:
            n = min(window, plan["file_bytes"] - first)
            ctx.seq_window(first, view[:n], times=t)
            if keep is not None:
                keep.append(view[:n].copy())
        return np.array(t["stitch"]), time.perf_counter() - t0

    counted, plain, clock = [], [], []
    for _ in range(warmup + reps):  # a walk behind a plan counts as it stitches ...
        ctx.seq_plan(plan)
        counted.append(walk()[0])
    comp_out = ctx.seq_out_composition(len(plan["names"]))
    for _ in range(warmup + reps):  # ... any later walk only stitches
        ms, dt = walk()
        plain.append(ms)
        clock.append(dt)
    counted, plain = np.array(counted[warmup:]), np.array(plain[warmup:])
    spread(passes, "stitch_counting_all_windows_ms", counted.sum(axis=1))
    spread(passes, "stitch_only_all_windows_ms", plain.sum(axis=1))
    spread(passes, "stitch_counting_per_full_window_ms", counted[:, :-1].ravel() if len(firsts) > 1 else counted.ravel())
    spread(passes, "stitch_only_per_full_window_ms", plain[:, :-1].ravel() if len(firsts) > 1 else plain.ravel())
    out["passes"] = passes
    out["host_clock"]["walk_all_windows_with_download_ms"] = round(1e3 * float(np.median(clock[warmup:])), 1)
    moved = plan["file_bytes"] + int(plan["body_len"].sum())  # every file byte written, every base read once
    for key in ("stitch_counting", "stitch_only"):
        sec = passes[key + "_all_windows_ms"] * 1e-3
        out["k_seq_" + key] = dict(bytes_moved=int(moved), bytes_per_second=round(moved / sec), share_of_measured_copy_rate=round(moved / sec / rate, 4))
    sec = passes["composition_ms"] * 1e-3
    out["k_seq_composition"] = dict(bytes_moved=int(buf.size), bytes_per_second=round(buf.size / sec), share_of_measured_copy_rate=round(buf.size / sec / (rate / 2.0), 4),
                                    note="a read-only pass: its share is of half the copy rate (the copy reads and writes)")
    ctx.seq_end()
    ctx.close()
    # the host rule on the same plan, and the two agree
    t0 = time.perf_counter()
    image, counts = sp.stitch(records, plan)
    t1 = time.perf_counter()
    comp_host = sp.composition(records)
    t2 = time.perf_counter()
    ctx = hip_lib.Context(0)
    parts = []
    sp.stitch_device(ctx, records, plan, lambda v: parts.append(bytes(v)), window=window)
    ctx.close()
    assert b"".join(parts) == image.tobytes() and np.array_equal(comp_out, counts) and np.array_equal(comp, comp_host), "the device and the rule disagree"
    del parts, image
    out["numpy_rule"] = dict(stitch_ms=round(1e3 * (t1 - t0), 1), composition_ms=round(1e3 * (t2 - t1), 1), agrees_with_the_device=True)
    # the whole call, the files in a memory-backed directory
    tmp = tempfile.mkdtemp(prefix="polish_bench_", dir=directory)
    try:
        fa, frags = os.path.join(tmp, "genome.fa"), os.path.join(tmp, "info_frags.txt")
        with open(fa, "wb") as fh:
            for name, seq in records:
                lines = np.frombuffer(seq[:len(seq) // 60 * 60], np.uint8).reshape(-1, 60)
                fh.write(b">" + name.encode() + b"\n" + np.concatenate((lines, np.full((lines.shape[0], 1), 10, np.uint8)), axis=1).tobytes() + seq[len(seq) // 60 * 60:] + b"\n")
        sp.write_info_frags(scaffolds, frags)
        whole = {}
        for device in (True, False):
            t, t0 = {}, time.perf_counter()
            r = sp.polish_assembly(frags, fa, os.path.join(tmp, "dev" if device else "host"), device=device, window=window, times=t)
            whole["device" if device else "host"] = dict(seconds=round(time.perf_counter() - t0, 2), read_fasta_s=round(t["read_s"], 2), list_work_s=round(t["lists_s"], 2),
                                                        stitch_and_write_s=round(t["stitch_s"], 2), kernels_ms=round(sum(t.get("stitch", [])) + sum(t.get("composition", [])), 2))
            whole["bases_lost"], whole["bases_duplicated"] = r["bases_lost"], r["bases_duplicated"]
        same = open(os.path.join(tmp, "dev", sp.POLISHED_GENOME_NAME), "rb").read() == open(os.path.join(tmp, "host", sp.POLISHED_GENOME_NAME), "rb").read()
        assert same, "the two folders differ"
        whole["folders_identical"] = True
        out["polish_assembly"] = whole
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=1_000_000_000)
    ap.add_argument("--records", type=int, default=24)
    ap.add_argument("--bins", type=int, default=200_000)
    ap.add_argument("--window", type=int, default=1 << 28)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default="/dev/shm", help="a memory-backed directory for the whole calls")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    doc = dict(what=("the polished FASTA of the polish step on one MI355X: the kernels under hipEvents, median of %d timed repetitions behind %d warm-ups, with the minimum and "
                     "the spread (max - min over the median); the whole polish_assembly call on the host clock with and without the device, the files in a "
                     "memory-backed directory (tools/polish_bench.py)" % (a.reps, a.warmup)))
    doc["result"] = measure(a.bases, a.records, a.bins, a.reps, a.warmup, a.window, a.dir)
    kit.write_doc(doc, a.out or next_profile())


if __name__ == "__main__":
    main()
