"""The entry points of the reader of 4DN pairs text (csrc/ig_host_text.inc): declared in include/instagraal_hip.h behind the pre block,
exported by the library, defined nowhere else, bound by hip_lib with the argument lists the header states, refusing NULL and
out-of-range arguments without a device, and reachable from every public call that takes a pairs path, whose defaults stay.  No GPU."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

from _abi_decl import assert_bound_as_declared as _assert_bound_as_declared, declaration as _declaration

ENTRY_POINTS = ("ig_text_begin", "ig_text_parse", "ig_text_fetch", "ig_text_feed_pre", "ig_text_feed_pairs", "ig_text_end")
N_ARGS = dict(ig_text_begin=5, ig_text_parse=6, ig_text_fetch=9, ig_text_feed_pre=3, ig_text_feed_pairs=2, ig_text_end=1)
EMPTY = inspect.Parameter.empty


def test_the_entry_points_are_declared_exported_and_bound_with_matching_signatures():
    from instagraal_amd import hip_lib, pairs_text

    hip_lib.build_lib()
    header = open(os.path.join(ROOT, "include", "instagraal_hip.h")).read()
    declared = set(re.findall(r"\b(ig_[a-z0-9_]+)\s*\(", header))
    assert set(ENTRY_POINTS) <= declared, sorted(set(ENTRY_POINTS) - declared)
    assert header.index("int ig_pre_end(") < header.index("int ig_text_begin(") < header.index("int ig_seq_begin(")
    import torch  # noqa: F401  (before the library, as hip_lib.lib() loads it: one HIP runtime per process)

    lib = ctypes.CDLL(hip_lib.LIB_PATH)
    assert not [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    csrc = os.path.join(ROOT, "instagraal_amd", "csrc")
    source = open(os.path.join(csrc, "ig_host_text.inc")).read()
    defined = set(re.findall(r'extern "C" int (ig_[a-z0-9_]+)\(', source))
    assert defined == set(ENTRY_POINTS), sorted(defined ^ set(ENTRY_POINTS))  # nothing exported that the header does not declare
    binding = open(os.path.join(ROOT, "instagraal_amd", "hip_lib.py")).read()
    for name in ENTRY_POINTS:
        decl = _declaration(header, name)
        assert len(decl) == N_ARGS[name] and decl[0] == "ig_ctx* ctx", (name, decl)
        defn = re.search(r'extern "C" int %s\(([^)]*)\)' % name, source).group(1).replace("\n", " ").split(",")
        strip = lambda a: re.sub(r"\s+", " ", a.strip())  # noqa: E731
        assert [strip(a).replace("ig_ctx* c", "ig_ctx* ctx") for a in defn] == [strip(a) for a in decl], name  # the definition is the declaration
        _assert_bound_as_declared(header, binding, name)
    for name in os.listdir(csrc):  # ... and defined nowhere else
        if name != "ig_host_text.inc":
            other = open(os.path.join(csrc, name)).read()
            assert not [n for n in ENTRY_POINTS if re.search(r'extern "C" int %s\(' % n, other)], name
    unit = open(os.path.join(csrc, "ig_hip.hip")).read()
    assert unit.index('"ig_kernels_text.cuh"') > unit.index('"ig_kernels_pre.cuh"')
    assert max(unit.index('"ig_host_pre.inc"'), unit.index('"ig_host_pairs.inc"')) < unit.index('"ig_host_text.inc"') < unit.index('"ig_host_batch.inc"')
    # one buffer struct on the handle, one free function, called in ig_destroy
    assert source.count("static void free_text_buffers(") == 1
    assert "free_text_buffers(c);" in open(os.path.join(csrc, "ig_host_core.inc")).read()
    common = open(os.path.join(csrc, "ig_common.cuh")).read()
    assert common.count("struct TextBuf {") == 1 and "TextBuf text;" in common
    kernels = open(os.path.join(csrc, "ig_kernels_text.cuh")).read()
    for k in ("k_text_mark", "k_text_lines", "k_text_parse", "k_text_compact", "k_text_convert"):
        assert re.search(r"__global__ void __launch_bounds__\(\w+\) %s\(" % k, kernels), k
    for used in ("(const uint4*)bytes", "__shared__ uint4 s_stage[TEXT_LDS_SPAN / 16 + 1]", "__shfl_up(", "atomicMin("):
        assert used in kernels, used
    for used in ("scan64_enqueue(", "pre_memory_guard(", "pre_add_impl(", "pairs_lift_staged(", "LiftTimer", "TEXT_UPLOAD_PIECE"):
        assert used in source, used
    assert "asm" not in kernels and "__builtin_amdgcn" not in kernels  # plain C++: ordinary vector loads, stores and atomics only
    # the constants the rule and the device share
    const = lambda k: int(re.search(r"#define TEXT_%s (\d+)" % k, kernels).group(1))  # noqa: E731
    assert (const("DATA"), const("COMMENT"), const("MALFORMED"), const("DEFERRED")) == (pairs_text.DATA, pairs_text.COMMENT, pairs_text.MALFORMED, pairs_text.DEFERRED)
    assert const("MAX_DIGITS") == 18 and "{1,18}" in pairs_text._INT.pattern.decode() and re.search(r"#define TEXT_MAX_BYTES \(1ll << 30\)", kernels)
    assert pairs_text.MAX_CHUNK_BYTES == 1 << 30 and pairs_text.DEFAULT_CHUNK_BYTES == 64 << 20
    assert const("LDS_SPAN") == const("LINES") * 128 and const("THREADS") == const("LINES") == 256
    assert re.search(r"#define TEXT_PASSES 4", source) and hip_lib.TEXT_PASSES == ("mark", "scan", "parse", "compact")
    assert len(pairs_text.SCALARS) == 8 and pairs_text.SCALARS[:7] == ("lines", "data", "comment", "malformed", "deferred", "first_columns_line", "to_host")
    for dep in ("ig_kernels_text.cuh", "ig_host_text.inc"):  # a change of either rebuilds the library
        assert any(d.endswith(dep) for d in hip_lib.DEPS)


def test_null_handles_are_refused_without_a_device():
    from instagraal_amd import hip_lib

    lib = hip_lib.lib()
    for name in ENTRY_POINTS:
        fn = getattr(lib, name)
        assert fn(*([None] + [0] * (len(fn.argtypes) - 1))) != 0, name
        assert b"NULL" in lib.ig_last_error() or b"null" in lib.ig_last_error(), (name, lib.ig_last_error())


def test_the_python_layers_reach_them_and_the_defaults_stay():
    from instagraal_amd import hip_lib, pairs_lift as pl, pairs_text as pt, pre
    from instagraal_amd.sampler import sampler
    from instagraal_amd.simulation import run_from_pairs

    for m in ("text_begin", "text_parse", "text_fetch", "text_feed_pre", "text_feed_pairs", "text_end"):
        assert callable(getattr(hip_lib.Context, m)), m
    params = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]  # noqa: E731
    assert params(pt.parse_chunk) == [("buf", EMPTY), ("cols", pt.DEFAULT_COLS), ("names", None)] and pt.DEFAULT_COLS == (1, 2, 3, 4, 5, 6)
    assert params(pt.complete) == [("res", EMPTY), ("buf", EMPTY), ("cols", EMPTY), ("names", EMPTY)]
    assert params(pt.read_pairs_bytes) == [("path", EMPTY), ("names", EMPTY), ("parse", None), ("chunk_bytes", pt.DEFAULT_CHUNK_BYTES)]
    assert [k for k, _ in params(pl.read_pairs_device)] == ["path", "names", "ctx", "chunk_bytes"]
    # the Python reader stays and stays the default: the device reader is asked for by name
    assert params(pl.read_pairs) == [("path", EMPTY), ("names", EMPTY), ("chunk_pairs", pl.DEFAULT_CHUNK_PAIRS), ("with_lines", False)]
    assert "reader" not in dict(params(pre.run_pre)) and [k for k, _ in params(run_from_pairs)] == ["fasta", "pairs", "enzymes", "output_folder", "run_kw"]
    assert params(pre.run_pre_reader) == [("fasta", EMPTY), ("pairs", EMPTY), ("enzymes", EMPTY), ("output_dir", EMPTY), ("reader", "host"), ("device", True), ("plot", False),
                                          ("chunk_pairs", pre.DEFAULT_CHUNK_PAIRS)]
    # the sampler's calls that take a pairs path keep their pinned parameter lists: the reader is the attribute pairs_reader
    assert sampler.pairs_reader == "host" and params(sampler._pairs_load)[-1] == ("reader", None)
    for f in (sampler.pairs_contacts, sampler.pairs_balance, sampler.write_pairs_zoom_levels, sampler.pairs_distance_law, sampler.display_pairs_distance_law):
        assert "reader" not in dict(params(f)), f.__name__
    assert "reader" not in dict(params(sampler.write_lifted_pairs)) and "reader" not in dict(params(pl.write_lifted_pairs))
    assert "Python reader" in pl.write_lifted_pairs.__doc__
