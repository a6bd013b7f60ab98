"""The host logic of the input folder from a FASTA and read pairs (csrc/ig_host_pre.inc) under AddressSanitizer / UBSan / LeakSanitizer
WITHOUT a GPU: the unmodified translation unit compiled with ``hipcc --offload-host-only -fsanitize=address,undefined`` and linked, as a
stand-alone program, against the fake HIP runtime of tests/sanitize/ and the models of tests/sanitize/pre_harness.cpp (one build for all
such tests: tests/_sanitize_build.py): the models do the kernels' loads and stores word for word, so the padding of the sequence, the
bitmaps and the fragment table are checked against the real allocation sizes and the digest against a brute force; the store growing
across chunks, every allocation failing once, ``begin`` twice, ``end`` without ``begin``, the refusals of the records and the sites, the
device errors the host must catch, a live session in front of ig_destroy, and a genome of four records across the coordinate 2^32
(4 GiB of host memory and as much "device" memory, about a minute): the 64-bit offsets and every size derived from them."""
import pytest

import _sanitize_build


def test_pre_host_logic_under_address_and_ub_sanitizers(tmp_path):
    if _sanitize_build.toolchain() is None:
        pytest.skip("no hipcc / clang++ / g++")
    r = _sanitize_build.build_and_run("pre_harness.cpp", "pre_asan", tmp_path)
    assert r.returncode == 0 and "pre harness ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
