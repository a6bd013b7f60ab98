"""The C ABI as include/instagraal_hip.h states it, read once: every ``ig_*`` declaration with its ctypes signature.

``hip_lib.lib()`` sets ``restype`` / ``argtypes`` of every entry point from here, so a call passes plain Python values and an argument of
the wrong C type raises ``ctypes.ArgumentError``.  The type map is closed: a type it does not know, or a statement it cannot read, is an
error when the library is loaded, never a guess.  No GPU, no library."""
import ctypes as C
import re
from collections import namedtuple

Param = namedtuple("Param", "text ctype")  # ``text``: the parameter as the header writes it, whitespace folded
Declaration = namedtuple("Declaration", "name returns restype params")

SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "void*": C.c_void_p, "const char*": C.c_char_p, "void": None}

_FUNCTION = re.compile(r"([\w \*]+?[\s\*])(ig_\w+)\s*\(([^()]*)\)\Z")
_SKIP = re.compile(r"typedef\s+struct\s+\w+(\s*\{[^{}]*\})?\s*\w+\Z")  # an opaque handle, or a struct the caller fills or reads


class HeaderError(ValueError):
    pass


def strip_comments(text):
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def _fold(c_type):
    """a C type in one spelling: single spaces, the stars against the type"""
    return re.sub(r"\s*\*\s*", "*", " ".join(c_type.split()))


def param_type(text):
    """the C type of one parameter, its name dropped; an array parameter is the pointer it decays to"""
    t, n_arrays = re.subn(r"\[[^\]]*\]", "", _fold(text))
    m = re.match(r"(.*?[\s\*])?(\w+)\Z", t)
    if m and m.group(1) and m.group(2) not in SCALARS and m.group(2) not in ("void", "char", "const"):
        t = m.group(1)  # the last word was the parameter's name
    return _fold(t) + "*" * n_arrays


def _ctype(c_type, where):
    if c_type == "const char*":
        return C.c_char_p
    if c_type.endswith("*"):
        return C.c_void_p
    if c_type not in SCALARS:
        raise HeaderError("%s: no ctypes type for '%s'" % (where, c_type))
    return SCALARS[c_type]


def declarations(header_text):
    """every ``ig_*`` function the header declares -> {name: Declaration}, in the header's order"""
    text = re.sub(r"^[ \t]*#[^\n]*(\\\n[^\n]*)*", " ", strip_comments(header_text), flags=re.M)  # preprocessor lines
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    out = {}
    statements = re.sub(r"(\{[^{}]*\})", lambda m: m.group(1).replace(";", "\0"), text).split(";")
    if statements[-1].strip() not in ("", "}"):  # ("}": the end of extern "C")
        raise HeaderError("cannot read the unterminated '%s'" % " ".join(statements[-1].split()))
    for statement in statements[:-1]:
        s = " ".join(statement.replace("\0", ";").split())
        if not s or _SKIP.match(s):
            continue
        m = _FUNCTION.match(s)
        if not m:
            raise HeaderError("cannot read the declaration '%s'" % s)
        returns, name, plist = _fold(m.group(1)), m.group(2), m.group(3).strip()
        if returns not in RETURNS:
            raise HeaderError("%s: no ctypes type for the return type '%s'" % (name, returns))
        if name in out:
            raise HeaderError("%s is declared twice" % name)
        texts = [] if plist in ("", "void") else [" ".join(p.split()) for p in plist.split(",")]
        if not all(texts):
            raise HeaderError("%s: an empty parameter in '%s'" % (name, plist))
        out[name] = Declaration(name, returns, RETURNS[returns], tuple(Param(p, _ctype(param_type(p), name)) for p in texts))
    missed = set(re.findall(r"\b(ig_\w+)\s*\(", text)) - set(out)
    if missed:
        raise HeaderError("named with '(' in the header but not read as declarations: %s" % ", ".join(sorted(missed)))
    return out


def apply(library, header_text):
    """set ``restype`` and ``argtypes`` of every declared function of a loaded library"""
    for d in declarations(header_text).values():
        fn = getattr(library, d.name)
        fn.restype, fn.argtypes = d.restype, [p.ctype for p in d.params]
