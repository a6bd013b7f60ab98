"""What the ABI tests read out of the sources: an entry point's declaration in the header and its one call in hip_lib.py."""
import re


def declaration(header, name):
    """the arguments of ``int <name>(...);`` in the header's text, one string each"""
    m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
    assert m, name
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


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
