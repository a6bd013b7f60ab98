"""The one sanitizer build of the host-logic harnesses (tests/sanitize/*_harness.cpp): the unmodified csrc/ig_hip.hip compiled host-only
under AddressSanitizer / UBSan, the fake HIP runtime and csrc/ig_draw.cpp -- once per Python process, in a temporary directory removed
at exit, never kept across sessions (an edited csrc/ cannot be tested through a stale object) -- and, per harness, its own object, the
link into a stand-alone program with its own main, and the run.  Nothing here is loaded into python.  Every compiler invocation is
appended to INVOCATIONS (and printed), so a session can count its library compiles."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SDIR = os.path.join(ROOT, "tests", "sanitize")
CSRC = os.path.join(ROOT, "instagraal_amd", "csrc")
SAN = ["-O1", "-g", "-std=c++17", "-fPIC", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
HOST = ["--offload-host-only", "-ffp-contract=off", "-Wno-unused-result", "-Wno-unused-value"] + SAN + ["-x", "hip"]
INVOCATIONS = []


def _call(cmd):
    INVOCATIONS.append(cmd)
    print("sanitize build:", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def toolchain():
    """(hipcc, clang++) when they and g++ are here, else None"""
    hipcc = shutil.which("hipcc")
    clangxx = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("amdclang++") or "") if p and os.path.exists(p)), None)
    if hipcc is None or clangxx is None or shutil.which("g++") is None:
        return None
    return hipcc, clangxx


@functools.lru_cache(maxsize=None)
def shared_objects():
    """the library object, the fake runtime's and the draw's, in the order they are linked behind a harness: the same in every harness"""
    hipcc, _ = toolchain()
    tmp = tempfile.mkdtemp(prefix="ig_sanitize_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    objs = {name: os.path.join(tmp, name + ".o") for name in ("lib", "fake", "draw")}
    _call([hipcc] + HOST + ["-c", os.path.join(CSRC, "ig_hip.hip"), "-o", objs["lib"]])
    _call([hipcc] + HOST + ["-c", os.path.join(SDIR, "fake_hip_runtime.cpp"), "-o", objs["fake"]])
    _call(["g++"] + SAN + ["-c", os.path.join(CSRC, "ig_draw.cpp"), "-o", objs["draw"]])
    return objs


def build_and_run(harness_cpp, exe_name, tmp_path, timeout=600):
    """tests/sanitize/<harness_cpp> linked against the shared objects as the program <exe_name>, run under the sanitizers: the completed
    process"""
    hipcc, clangxx = toolchain()
    shared = shared_objects()
    harness = str(tmp_path / "harness.o")
    _call([hipcc] + HOST + ["-c", os.path.join(SDIR, harness_cpp), "-o", harness])
    objs = [shared["lib"], shared["fake"], harness, shared["draw"]]
    # the host-side registration code refers to the (absent) device binary by a hashed symbol: never dereferenced by the fake runtime
    undefined = subprocess.run(["nm", "-u"] + objs, capture_output=True, text=True, check=True).stdout
    fatbins = sorted({w for w in undefined.split() if w.startswith("__hip_fatbin")})
    exe = str(tmp_path / exe_name)
    _call([clangxx, "-fsanitize=address,undefined", "-o", exe] + objs + ["-Wl,--defsym=%s=0" % f for f in fatbins] + ["-lpthread"])
    return subprocess.run([exe], capture_output=True, text=True, timeout=timeout,
                          env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
