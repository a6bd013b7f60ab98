"""The host logic of the balancing's rows from a built map (csrc/ig_host_balsnap.inc: the build from the resident snapshot, the debug
entry over caller data, the timed entry, every refusal, the lifetimes of the snapshot and the rows through build / rows / run / release
/ coarsen) under AddressSanitizer / UBSan / LeakSanitizer WITHOUT a GPU: the unmodified translation unit compiled with
``hipcc --offload-host-only -fsanitize=address,undefined`` and linked, as a stand-alone program, against the fake HIP runtime of
tests/sanitize/ and the word-for-word kernel models of tests/sanitize/balsnap_harness.cpp (one build for all such tests:
tests/_sanitize_build.py)."""
import pytest

import _sanitize_build


def test_balance_snapshot_host_logic_under_address_and_ub_sanitizers(tmp_path):
    if _sanitize_build.toolchain() is None:
        pytest.skip("no hipcc / clang++ / g++")
    r = _sanitize_build.build_and_run("balsnap_harness.cpp", "balsnap_asan", tmp_path)
    assert r.returncode == 0 and "balsnap harness ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
