"""The host logic of the gap support (csrc/ig_host_gap.inc) under AddressSanitizer / UBSan / LeakSanitizer WITHOUT a GPU:
the unmodified translation unit compiled with ``hipcc --offload-host-only -fsanitize=address,undefined`` and linked, as a stand-alone
program, against the fake HIP runtime of tests/sanitize/ and the models of tests/sanitize/gap_harness.cpp (built as
tests/test_orientation_support_sanitize.py builds the orientation support's harness)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_gap_support_host_logic_under_address_and_ub_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc")
    clangxx = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("amdclang++") or "") if p and os.path.exists(p)), None)
    if hipcc is None or clangxx is None or shutil.which("g++") is None:
        pytest.skip("no hipcc / clang++ / g++")
    san = ["-O1", "-g", "-std=c++17", "-fPIC", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    host = [hipcc, "--offload-host-only", "-ffp-contract=off", "-Wno-unused-result", "-Wno-unused-value"] + san
    sdir = os.path.join(ROOT, "tests", "sanitize")
    objs = {}
    for name, src in (("lib", os.path.join(ROOT, "instagraal_amd", "csrc", "ig_hip.hip")), ("fake", os.path.join(sdir, "fake_hip_runtime.cpp")),
                      ("harness", os.path.join(sdir, "gap_harness.cpp"))):
        objs[name] = str(tmp_path / (name + ".o"))
        subprocess.check_call(host + ["-x", "hip", "-c", src, "-o", objs[name]])
    objs["draw"] = str(tmp_path / "draw.o")
    subprocess.check_call(["g++"] + san + ["-c", os.path.join(ROOT, "instagraal_amd", "csrc", "ig_draw.cpp"), "-o", objs["draw"]])
    # the host-side registration code refers to the (absent) device binary by a hashed symbol: never dereferenced by the fake runtime
    undefined = subprocess.run(["nm", "-u"] + list(objs.values()), capture_output=True, text=True, check=True).stdout
    fatbins = sorted({w for w in undefined.split() if w.startswith("__hip_fatbin")})
    exe = str(tmp_path / "gap_asan")
    subprocess.check_call([clangxx, "-fsanitize=address,undefined", "-o", exe] + list(objs.values()) + ["-Wl,--defsym=%s=0" % f for f in fatbins] + ["-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "gap harness ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
