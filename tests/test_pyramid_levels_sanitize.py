"""The host logic of the pyramid's contact levels (csrc/ig_host_pyr.inc) under AddressSanitizer / UBSan / LeakSanitizer WITHOUT a GPU:
the unmodified translation unit compiled with ``hipcc --offload-host-only -fsanitize=address,undefined`` and linked, as a stand-alone
program, against the fake HIP runtime of tests/sanitize/ and the models of tests/sanitize/pyr_harness.cpp (one build for all such
tests: tests/_sanitize_build.py): the models do the kernels' loads and stores word for word, so the list, the table of a remap, the
degrees and the fetched stretches are checked against the real allocation sizes and every level against a brute force; the upload
in pieces, the two RowBufs swapping over three levels, every allocation failing once, ``begin`` twice, ``end`` without ``begin``, every
refusal, the device errors the host must catch, and a live session in front of ig_destroy.  Nothing is loaded into Python."""
import pytest

import _sanitize_build


def test_pyr_host_logic_under_address_and_ub_sanitizers(tmp_path):
    if _sanitize_build.toolchain() is None:
        pytest.skip("no hipcc / clang++ / g++")
    r = _sanitize_build.build_and_run("pyr_harness.cpp", "pyr_asan", tmp_path)
    assert r.returncode == 0 and "pyr harness ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
