"""The host logic of the segment placement support (csrc/ig_host_segplace.inc) under AddressSanitizer / UBSan / LeakSanitizer WITHOUT a
GPU: the unmodified translation unit compiled with ``hipcc --offload-host-only -fsanitize=address,undefined`` and linked, as a stand-alone
program, against the fake HIP runtime of tests/sanitize/ and the models of tests/sanitize/segplace_harness.cpp
(one build for all such tests: tests/_sanitize_build.py)."""
import pytest

import _sanitize_build


def test_segment_placement_host_logic_under_address_and_ub_sanitizers(tmp_path):
    if _sanitize_build.toolchain() is None:
        pytest.skip("no hipcc / clang++ / g++")
    r = _sanitize_build.build_and_run("segplace_harness.cpp", "segplace_asan", tmp_path)
    assert r.returncode == 0 and "segplace harness ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
