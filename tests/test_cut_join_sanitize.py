"""The host logic of the cut and join scores (csrc/ig_host_cutjoin.inc) under AddressSanitizer / UBSan / LeakSanitizer WITHOUT a GPU: the
unmodified translation unit compiled with ``hipcc --offload-host-only -fsanitize=address,undefined`` and linked, as a stand-alone
program, against the fake HIP runtime of tests/sanitize/ and the models of tests/sanitize/cutjoin_harness.cpp (one build for all such
tests: tests/_sanitize_build.py): genomes of other shapes on one handle (contigs of 1, 2, 7 and 40 bins, a ring), pairs on both sides of
the LDS window in both forms of the pass, the prefix table of the zero-pixel terms, the device errors the host must catch, the refusals,
every allocation failing once, the host-only entries, and a live result in front of ig_destroy."""
import pytest

import _sanitize_build


def test_cut_join_host_logic_under_address_and_ub_sanitizers(tmp_path):
    if _sanitize_build.toolchain() is None:
        pytest.skip("no hipcc / clang++ / g++")
    r = _sanitize_build.build_and_run("cutjoin_harness.cpp", "cutjoin_asan", tmp_path)
    assert r.returncode == 0 and "cutjoin harness ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
