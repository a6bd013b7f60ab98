"""The host logic of the segment edits (csrc/ig_host_edit.inc) under AddressSanitizer / UBSan / LeakSanitizer WITHOUT a GPU: the
unmodified translation unit compiled with ``hipcc --offload-host-only -fsanitize=address,undefined`` and linked, as a stand-alone
program, against the fake HIP runtime of tests/sanitize/ and the models of tests/sanitize/rearrange_harness.cpp (one build for all such
tests: tests/_sanitize_build.py): the chunking of a list at 1, 64, 65 and 130 edits and under a memory limit, the refusals, the reuse of
the buffers across calls with growing and shrinking lists and with a state of fewer, then again more bins (the number of
sub-fragments of a handle cannot change once the contacts are uploaded)."""
import pytest

import _sanitize_build


def test_segment_edits_host_logic_under_address_and_ub_sanitizers(tmp_path):
    if _sanitize_build.toolchain() is None:
        pytest.skip("no hipcc / clang++ / g++")
    r = _sanitize_build.build_and_run("rearrange_harness.cpp", "rearrange_asan", tmp_path)
    assert r.returncode == 0 and "rearrange harness ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
