"""The host logic of the placement support (csrc/ig_host_place.inc), of the records it shares with the join support and of the sort and
reduction it shares with the contacts in genome coordinates, under AddressSanitizer / UBSan / LeakSanitizer WITHOUT a GPU: the
unmodified translation unit compiled with ``hipcc --offload-host-only -fsanitize=address,undefined`` and linked, as a stand-alone
program, against the fake HIP runtime of tests/sanitize/ and the models of tests/sanitize/place_harness.cpp
(one build for all such tests: tests/_sanitize_build.py)."""
import pytest

import _sanitize_build


def test_placement_support_host_logic_under_address_and_ub_sanitizers(tmp_path):
    if _sanitize_build.toolchain() is None:
        pytest.skip("no hipcc / clang++ / g++")
    r = _sanitize_build.build_and_run("place_harness.cpp", "place_asan", tmp_path)
    assert r.returncode == 0 and "place harness ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
