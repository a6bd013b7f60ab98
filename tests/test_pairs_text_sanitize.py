"""The host logic of the reader of 4DN pairs text (csrc/ig_host_text.inc) under AddressSanitizer / UBSan / LeakSanitizer WITHOUT a GPU:
the unmodified translation unit compiled host-only and linked, as a stand-alone program, against the fake HIP runtime of tests/sanitize/
and the models of tests/sanitize/text_harness.cpp (one build for all such tests: tests/_sanitize_build.py).  The models do the kernels'
loads and stores word for word, so the two 16-byte loads of the last run and the staging of a workgroup's lines are checked against the
real allocation sizes, and the result against a line-by-line brute force; the buffers growing across chunks, every allocation failing
once, ``begin`` twice, ``end`` without ``begin``, the refusals on the arguments, and a live session in front of ig_destroy."""
import pytest

import _sanitize_build


def test_pairs_text_host_logic_under_address_and_ub_sanitizers(tmp_path):
    if _sanitize_build.toolchain() is None:
        pytest.skip("no hipcc / clang++ / g++")
    r = _sanitize_build.build_and_run("text_harness.cpp", "text_asan", tmp_path)
    assert r.returncode == 0 and "text harness ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
