"""The host tests' one reader of include/vitamd.h.  It shares no code with the parser of vitamd/lib.py on purpose: the argument counts the
tests write out (`== 18`, `== 13`, ...) and the names they look up here check that parser from the outside."""
import functools
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vitamd.h")
_DECL = re.compile(r"\b(int|long)\s+(vitamd_\w+)\s*\(([^;]*?)\)\s*;", re.S)


@functools.lru_cache(maxsize=None)
def header():
    """the text of the header, comments included"""
    with open(HEADER) as fh:
        return fh.read()


@functools.lru_cache(maxsize=None)
def _declarations():
    return {name: (ret, params) for ret, name, params in _DECL.findall(header())}


def declared():
    """({name: parameter count}, {name: "int" or "long"}) over every entry point the header declares"""
    decls = _declarations()
    counts = {name: (0 if params.strip() in ("", "void") else params.count(",") + 1) for name, (_, params) in decls.items()}
    return counts, {name: ret for name, (ret, _) in decls.items()}


def declaration(name):
    """the parameter list of one declaration, as written between its parentheses (KeyError: not declared)"""
    return _declarations()[name][1]
