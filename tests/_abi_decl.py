"""What the ABI tests read out of the sources: an entry point's declaration in the header (``instagraal_amd.abi``, the parser the binding
itself loads its signatures with) and its one call in hip_lib.py."""
import functools

from instagraal_amd import abi

declarations = functools.lru_cache(maxsize=None)(abi.declarations)


def declaration(header, name):
    """the parameters of ``<name>`` as the header's text declares them, one string each"""
    return [p.text for p in declarations(header)[name].params]


def call_args(source, name):
    """the arguments of the first call of ``lib().<name>(`` in the binding's text, split at the top level"""
    start = "lib().%s(" % name
    i = source.index(start) + len(start)
    depth, args, cur = 1, [], ""
    while depth:
        ch = source[i]
        depth += (ch in "([") - (ch in ")]")
        if depth == 1 and ch == ",":
            args.append(cur.strip())
            cur = ""
        elif depth:
            cur += ch
        i += 1
    return args + [cur.strip()]


def assert_bound_as_declared(header, binding, name):
    """the loaded library's function carries the header's types, and the binding's call passes one argument for each, the handle first"""
    from instagraal_amd import hip_lib

    decl, fn = declarations(header)[name], getattr(hip_lib.lib(), name)
    assert fn.restype is decl.restype and list(fn.argtypes) == [p.ctype for p in decl.params], (name, fn.restype, fn.argtypes)
    call = call_args(binding, name)
    assert len(call) == len(decl.params) and call[0] == "self._h", (name, call)
