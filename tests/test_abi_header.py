"""The C ABI has one owner, include/instagraal_hip.h: ``instagraal_amd.abi`` reads every declaration out of it, ``hip_lib.lib()`` gives every
entry point those types, every definition under csrc/ has them, and every call of the binding passes that many arguments -- for all the
entry points the header declares, not for a list kept by hand.  No GPU."""
import ctypes as C
import glob
import os
import re

import pytest
from conftest import ROOT

from _abi_decl import call_args, declarations
from instagraal_amd import abi

HEADER = open(os.path.join(ROOT, "include", "instagraal_hip.h")).read()
# the type map, stated a second time on purpose: what the parser and the loader make of the header is held against it
SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "void*": C.c_void_p, "const char*": C.c_char_p, "void": None}
STAR_CALLS = {"ig_placement_support", "ig_join_scores_fetch"}  # the only calls that build a part of their argument list: counted below


def _want(param):
    t = abi.param_type(param)
    return C.c_char_p if t == "const char*" else C.c_void_p if t.endswith("*") else SCALARS[t]


def _types_only(c_types):  # const and whitespace normalised
    return [re.sub(r"\bconst\b", "", t).replace(" ", "") for t in c_types]


def test_the_parser_reads_every_declaration_and_the_library_carries_it():
    from instagraal_amd import hip_lib

    decls = declarations(HEADER)
    loose = set(re.findall(r"\b(ig_[a-z0-9_]+)\s*\(", HEADER))  # test_library_exports_every_declared_symbol's
    assert set(decls) == loose and len(decls) >= 191, sorted(set(decls) ^ loose)
    assert [abi.param_type(t) for t in ("ig_ctx** out", "const int32_t *row", "int64_t out4[4]", "void* s", "int32_t", "const char* path")] == \
        ["ig_ctx**", "const int32_t*", "int64_t*", "void*", "int32_t", "const char*"]
    assert [(p.text, p.ctype) for p in decls["ig_set_params"].params] == [("ig_ctx* ctx", C.c_void_p), ("const float p[8]", C.c_void_p),
                                                                         ("float mean_subfrag_kb", C.c_float), ("int which", C.c_int32)]
    hip_lib.build_lib()
    lib = hip_lib.lib()
    for d in decls.values():
        want = [_want(p.text) for p in d.params]
        assert d.restype is RETURNS[d.returns] and [p.ctype for p in d.params] == want, d
        assert getattr(lib, d.name).restype is d.restype and list(getattr(lib, d.name).argtypes) == want, d.name
    assert list(lib.ig_last_error.argtypes) == [] and lib.ig_destroy.restype is None and lib.ig_partials_count.restype is C.c_int64
    assert hip_lib.DEPS[-1] == hip_lib.HEADER and os.path.samefile(hip_lib.HEADER, os.path.join(ROOT, "include", "instagraal_hip.h"))
    for wrong in (C.c_int64(1), 1.0):  # the wrong C type is refused, where it used to reach the library as it came
        with pytest.raises(C.ArgumentError):
            lib.ig_set_batch_width(wrong)


@pytest.mark.parametrize("line", ["int ig_made_up(ig_ctx* ctx, long n);", "long ig_made_up(ig_ctx* ctx);",  # types outside the map
                                  "int ig_made_up(int32_t n), ig_other(int32_t n);", "int (*ig_made_up)(int32_t n);",  # shapes it cannot read
                                  "static inline int ig_made_up(int32_t n) { return n; }", "int ig_made_up(int32_t n)"])
def test_the_parser_refuses_what_it_does_not_know(line):
    with pytest.raises(abi.HeaderError, match="ig_made_up"):
        abi.declarations(HEADER.replace("int ig_sync(", line + "\nint ig_sync("))
    assert "ig_made_up" not in abi.declarations(HEADER.replace("int ig_sync(", "/* " + line + " */\nint ig_sync("))  # a comment declares nothing


def test_every_entry_point_is_defined_once_with_the_declared_types():
    found = {}
    for path in glob.glob(os.path.join(ROOT, "instagraal_amd", "csrc", "*")):
        for m in re.finditer(r'extern\s+"C"\s+([\w \*]+?[\s\*])(ig_\w+)\s*\(([^()]*)\)\s*\{', abi.strip_comments(open(path).read())):
            found.setdefault(m.group(2), []).append((m.group(1), m.group(3).strip()))
    decls = declarations(HEADER)
    assert set(found) == set(decls), sorted(set(found) ^ set(decls))
    for name, d in decls.items():
        assert len(found[name]) == 1, (name, found[name])
        returns, plist = found[name][0]
        params = [] if plist in ("", "void") else [abi.param_type(p) for p in plist.split(",")]
        assert _types_only([returns]) == _types_only([d.returns]), (name, returns)
        assert _types_only(params) == _types_only(abi.param_type(p.text) for p in d.params), (name, params)


def test_every_call_of_the_binding_passes_the_declared_number_of_arguments():
    """ctypes refuses too few arguments and lets extra ones through: the count is held here"""
    from instagraal_amd import hip_lib, placement_support

    binding = open(os.path.join(ROOT, "instagraal_amd", "hip_lib.py")).read()
    decls = declarations(HEADER)
    tuples = dict(INT_ARRAYS=placement_support.INT_ARRAYS, LONG_ARRAYS=placement_support.LONG_ARRAYS, CONTIG_ARRAYS=hip_lib.CONTIG_ARRAYS)
    called, starred = set(), set()
    for m in re.finditer(r"lib\(\)\.(ig_\w+)\(", binding):
        name = m.group(1)
        call = [a for a in call_args(binding[m.start():], name) if a]
        n = len(call)
        for a in call:
            if a.startswith("*"):  # one address per name of tuples that need no device to be counted
                starred.add(name)
                n += len(eval(re.fullmatch(r"\*\[_p\(out\[k\]\) for k in (.+)\]", a).group(1), dict(tuples))) - 1
        assert n == len(decls[name].params), (name, call)
        called.add(name)
    assert starred == STAR_CALLS and set(decls) - called == {"ig_debug_set_tail_quirk"}  # (declared, exported and left unbound)
    assert not re.findall(r"\.ig_\w+", binding.replace("lib().ig_", ""))  # and the library is called in no other way
