"""The host logic of the fixed-resolution maps (csrc/ig_host_zoom.inc: the lift and the balancing's build with a caller's units, the
coarsening of a built level, the debug entries, every refusal, the snapshot's lifetime) under AddressSanitizer / UBSan / LeakSanitizer
WITHOUT a GPU: the unmodified translation unit compiled with ``hipcc --offload-host-only -fsanitize=address,undefined`` and linked, as a
stand-alone program, against the fake HIP runtime of tests/sanitize/ and the models of tests/sanitize/zoom_harness.cpp (one build for
all such tests: tests/_sanitize_build.py)."""
import pytest

import _sanitize_build


def test_zoom_levels_host_logic_under_address_and_ub_sanitizers(tmp_path):
    if _sanitize_build.toolchain() is None:
        pytest.skip("no hipcc / clang++ / g++")
    r = _sanitize_build.build_and_run("zoom_harness.cpp", "zoom_asan", tmp_path)
    assert r.returncode == 0 and "zoom harness ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
