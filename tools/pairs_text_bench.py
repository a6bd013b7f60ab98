#!/usr/bin/env python3
"""The reader of 4DN pairs text on the device (ig_text_begin, ig_text_parse, ig_text_fetch, ig_text_feed_pre,
csrc/ig_kernels_text.cuh) timed -> the next free profiles/rNN_pairs_text.json.

On a seeded pairs text of ``--lines`` lines made in memory (24 contigs, 80 % of the pairs on one contig, both strands):
  * the four passes of ``ig_text_parse`` under hipEvents over the text in chunks of ``--chunk-bytes``: the sum over the chunks per
    repetition, its median behind the warm-ups, with the minimum and the spread (the largest minus the smallest sample over the median);
  * the bytes of the text over the time of the four passes, against the device-to-device copy rate measured in the same run;
  * the whole ``read_pairs_device`` on a plain file and on a ``.gz`` on the host clock, split into read / inflate (``pairs_text.blocks``
    alone), upload with the passes (``text_parse`` on the host clock less nothing: the copy is inside the call), fetch and completion;
  * ``read_pairs`` -- the Python line loop, the reader before this one and the baseline -- on ``--baseline-lines`` lines of the same
    text, extrapolated linearly and labelled as such;
  * the whole ``run_pre`` with both readers on one input of ``--run-pre-lines`` lines, their dicts compared.

  python tools/pairs_text_bench.py [--lines 10000000] [--out profiles/rNN_pairs_text.json]
"""
import argparse
import glob
import gzip
import os
import re
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import numpy as np

import _report_bench as kit
import pre_bench


def next_profile():
    taken = [int(m.group(1)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*_*")) for m in [re.match(r"r(\d+)_", os.path.basename(p))] if m]
    return os.path.join(ROOT, "profiles", "r%02d_pairs_text.json" % (max(taken, default=0) + 1))


def seeded_text(lens, names, n_lines, seed=3, piece=1_000_000):
    """-> bytes: a header and n_lines lines ``readID chr1 pos1 chr2 pos2 strand1 strand2``, the pairs of ``pre_bench.seeded_pairs``"""
    c1, p1, c2, p2 = pre_bench.seeded_pairs(lens, n_lines, seed)
    st = np.random.default_rng(seed).integers(0, 4, n_lines)
    out = [b"## pairs format v1.0\n#columns: readID chr1 pos1 chr2 pos2 strand1 strand2\n"]
    for a in range(0, n_lines, piece):
        rows = zip(range(a, min(a + piece, n_lines)), c1[a:a + piece].tolist(), p1[a:a + piece].tolist(), c2[a:a + piece].tolist(), p2[a:a + piece].tolist(), st[a:a + piece].tolist())
        out.append("".join("SRR0000001.%d\t%s\t%d\t%s\t%d\t%s\t%s\n" % (k, names[x], p, names[y], q, "+-"[s & 1], "+-"[s >> 1]) for k, x, p, y, q, s in rows).encode())
    return b"".join(out)


def first_lines(text, n):
    """the header's two lines and the first n data lines"""
    nl = np.flatnonzero(np.frombuffer(text, np.uint8)[:(n + 3) * 256] == 10)
    return text[:int(nl[n + 1]) + 1]


def clock(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t0)


def measure(a):
    from instagraal_amd import hip_lib, pairs_lift as pl, pairs_text as pt, pre

    records = pre_bench.seeded_genome(a.bases, 24)
    names = [n for n, _ in records]
    ids = {n: k for k, n in enumerate(names)}
    lens = [len(s) for _, s in records]
    text = seeded_text(lens, names, a.lines)
    out = dict(lines=a.lines, text_bytes=len(text), bytes_per_line=round(len(text) / a.lines, 1), chunk_bytes=a.chunk_bytes, contigs=len(names))
    rate = pre_bench.copy_rate()
    out["hbm_copy_bytes_per_second_measured"] = round(rate)
    ctx = hip_lib.Context(0)
    # ---- the passes, chunk by chunk as the reader cuts them
    head = text.index(b"\n", text.index(b"#columns:")) + 1
    cuts, at = [], head
    while at < len(text):
        end = min(at + a.chunk_bytes, len(text))
        end = text.rfind(b"\n", at, end) + 1 if end < len(text) else end
        cuts.append((at, end))
        at = end
    view = np.frombuffer(text, np.uint8)
    ctx.text_begin(ids)
    ms, counts = [], None
    for r in range(a.warmup + a.reps):
        tot, got = np.zeros(len(hip_lib.TEXT_PASSES)), dict(lines=0, data=0, deferred=0, malformed=0)
        for lo, hi in cuts:
            res = ctx.text_parse(view[lo:hi], times=True)
            tot += res["ms"]
            assert not res["to_host"]
            for k in got:
                got[k] += res["counts"][k]
        ms.append(tot)
        counts = got
    assert counts == dict(lines=a.lines, data=a.lines, deferred=0, malformed=0), counts
    ms = np.array(ms[a.warmup:])
    passes = {}
    for k, name in enumerate(hip_lib.TEXT_PASSES):
        pre_bench.spread(passes, name + "_ms", ms[:, k])
    pre_bench.spread(passes, "all_ms", ms.sum(axis=1))
    out["passes"] = passes
    n_body = len(text) - head
    out["parse"] = dict(bytes_per_second=round(n_body / (passes["all_ms"] * 1e-3)), lines_per_second=round(a.lines / (passes["all_ms"] * 1e-3)),
                        share_of_measured_copy_rate=round(n_body / (passes["all_ms"] * 1e-3) / rate, 4),
                        note="the copy rate moves every byte twice (read + write); the passes read the text about twice (mark, parse) and write 26 bytes a line")
    ctx.text_end()
    # ---- the whole reader on files, on the host clock
    host = {}
    with tempfile.TemporaryDirectory() as tmp:
        plain, gz = os.path.join(tmp, "in.pairs"), os.path.join(tmp, "in.pairs.gz")
        with open(plain, "wb") as f:
            f.write(text)
        with gzip.open(gz, "wb", compresslevel=1) as f:
            f.write(text)
        out["gz_bytes"] = os.path.getsize(gz)
        for what, path in (("plain", plain), ("gz", gz)):
            _, t_read = clock(lambda: sum(len(b) for b in pt.blocks(path, a.chunk_bytes)))
            split = dict(parse=0.0, fetch=0.0)

            def parse(seg, cols):
                res, t = clock(lambda: ctx.text_parse(seg, cols))
                split["parse"] += t
                res, t = clock(lambda: ctx.text_fetch(res))
                split["fetch"] += t
                return res

            ctx.text_begin(ids)
            n, t_all = clock(lambda: sum(ch["c1"].size for ch in pt.read_pairs_bytes(path, ids, parse, a.chunk_bytes)))
            ctx.text_end()
            assert n == a.lines
            host[what] = dict(read_pairs_device_ms=round(t_all, 1), read_or_inflate_alone_ms=round(t_read, 1), upload_and_passes_ms=round(split["parse"], 1),
                              fetch_ms=round(split["fetch"], 1), completion_and_concatenation_ms=round(t_all - t_read - split["parse"] - split["fetch"], 1),
                              lines_per_second=round(a.lines / (t_all * 1e-3)))
        # ---- the baseline: the Python line loop, on a part of the same text
        part = os.path.join(tmp, "part.pairs")
        with open(part, "wb") as f:
            f.write(first_lines(text, a.baseline_lines))
        n, t_base = clock(lambda: sum(ch["c1"].size for ch in pl.read_pairs(part, ids)))
        assert n == a.baseline_lines
        out["read_pairs_baseline"] = dict(lines=n, seconds=round(t_base * 1e-3, 3), lines_per_second=round(n / (t_base * 1e-3)), extrapolated_to_lines=a.lines,
                                          extrapolated_seconds=round(t_base * 1e-3 * a.lines / n, 1),
                                          note="pairs_lift.read_pairs, the reader before this one, on the CPU this was run on; extrapolated linearly, not measured at that count")
        # ---- the whole run_pre with both readers on one input
        fasta, sub = os.path.join(tmp, "g.fa"), os.path.join(tmp, "sub.pairs")
        with open(fasta, "wb") as f:
            f.write(b"".join(b">%s\n%s\n" % (n_.encode(), s) for n_, s in records))
        with open(sub, "wb") as f:
            f.write(first_lines(text, a.run_pre_lines))
        r_host, t_host = clock(lambda: pre.run_pre(fasta, sub, list(pre_bench.ENZYMES), os.path.join(tmp, "host"), device=ctx))
        r_dev, t_dev = clock(lambda: pre.run_pre_reader(fasta, sub, list(pre_bench.ENZYMES), os.path.join(tmp, "dev"), device=ctx, reader="device"))
        same = r_host == r_dev and all(open(os.path.join(tmp, "host", f), "rb").read() == open(os.path.join(tmp, "dev", f), "rb").read()
                                       for f in ("fragments_list.txt", "info_contigs.txt", "abs_fragments_contacts_weighted.txt"))
        assert same, "run_pre differs between the readers"
        out["run_pre"] = dict(lines=a.run_pre_lines, bases=int(sum(lens)), reader_host_ms=round(t_host, 1), reader_device_ms=round(t_dev, 1), same_files_and_dict=True,
                              note="the FASTA read, the digest, the pixels and the three text files written are in both")
    out["host_clock"] = host
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--bases", type=int, default=50_000_000)
    ap.add_argument("--chunk-bytes", type=int, default=64 << 20)
    ap.add_argument("--baseline-lines", type=int, default=100_000)
    ap.add_argument("--run-pre-lines", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    doc = dict(what=("the reader of 4DN pairs text on one MI355X: the four passes under hipEvents summed over the chunks, median of %d timed repetitions behind %d "
                     "warm-ups, with the minimum and the spread (max - min over the median); the whole reader, the Python baseline and run_pre on the host clock, once "
                     "each (tools/pairs_text_bench.py)" % (a.reps, a.warmup)))
    doc["result"] = measure(a)
    kit.write_doc(doc, a.out or next_profile())


if __name__ == "__main__":
    main()
