"""The host logic of the read pairs lifted onto the current genome (csrc/ig_host_pairs.inc) under AddressSanitizer / UBSan /
LeakSanitizer WITHOUT a GPU: the unmodified translation unit compiled with ``hipcc --offload-host-only -fsanitize=address,undefined`` and
linked, as a stand-alone program, against the fake HIP runtime of tests/sanitize/ and the models of tests/sanitize/pairs_harness.cpp (one
build for all such tests: tests/_sanitize_build.py): the store growing across chunks, every allocation failing once, ``begin`` twice,
``end`` without ``begin``, the refusals of the table, the pixels and the law, a session across a new state, the device errors the host
must catch, and a live session in front of ig_destroy."""
import pytest

import _sanitize_build


def test_pairs_host_logic_under_address_and_ub_sanitizers(tmp_path):
    if _sanitize_build.toolchain() is None:
        pytest.skip("no hipcc / clang++ / g++")
    r = _sanitize_build.build_and_run("pairs_harness.cpp", "pairs_asan", tmp_path)
    assert r.returncode == 0 and "pairs harness ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
