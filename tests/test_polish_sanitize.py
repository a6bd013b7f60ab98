"""The host logic of the polished FASTA of the polish step (csrc/ig_host_seq.inc) under AddressSanitizer / UBSan / LeakSanitizer WITHOUT
a GPU: the unmodified translation unit compiled with ``hipcc --offload-host-only -fsanitize=address,undefined`` and linked, as a
stand-alone program, against the fake HIP runtime of tests/sanitize/ and tests/sanitize/seq_harness.cpp (one build for all such tests:
tests/_sanitize_build.py).  The harness runs the per-thread functions of csrc/ig_kernels_seq.cuh themselves over the fake device heap, in
the kernels' order, so every load around the first and the last base of the sequence and every store of a window is checked against
the real allocation sizes and the file against a per-bin string build; every refusal of ``ig_seq_plan``, of the windows and of the
records; every allocation failing once; a live session in front of ig_destroy; and a plan whose file offsets cross 2^32 (pieces that
use one record of 4 MiB again and again: the plan arithmetic and small windows on either side, nothing of 4 GiB exists)."""
import pytest

import _sanitize_build


def test_seq_host_logic_under_address_and_ub_sanitizers(tmp_path):
    if _sanitize_build.toolchain() is None:
        pytest.skip("no hipcc / clang++ / g++")
    r = _sanitize_build.build_and_run("seq_harness.cpp", "seq_asan", tmp_path)
    assert r.returncode == 0 and "seq harness ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
