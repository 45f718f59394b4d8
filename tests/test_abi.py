"""The C ABI, stated twice by hand -- include/grl_hip.h and the ctypes mirrors and signature table of _lib.py -- compared in
full on the CPU: every struct and field (gcc's sizeof / offsetof), the version macros, and every prototype.  Structs are found by
introspection and prototypes by parsing the header, so a new entry point is covered without an edit here."""
import ctypes as C
import os
import re
import subprocess

import pytest

from grl_image_restoration_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "grl_hip.h")


def _header_code() -> str:
    """The header without its comments (they quote prototypes and struct names)."""
    text = open(HEADER).read()
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def _mirrors() -> dict:
    return {name: t for name, t in vars(_lib).items()
            if isinstance(t, type) and issubclass(t, _lib._Strict) and t is not _lib._Strict}


@pytest.fixture(scope="module")
def compiled(tmp_path_factory) -> dict:
    """What gcc makes of the header: `<Struct>` -> sizeof, `<Struct>.<field>` -> (offsetof, sizeof), and the two macros."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "grl_hip.h"', "int main(void) {"]
    for name, st in _mirrors().items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for field, _ in st._fields_:
            lines.append(f'printf("{name}.{field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name}*)0)->{field}));')
    lines += ['printf("GRL_ABI_VERSION %d\\n", (int)GRL_ABI_VERSION);', 'printf("GRL_METRIC_COUNT %d\\n", (int)GRL_METRIC_COUNT);',
              "return 0; }"]
    d = tmp_path_factory.mktemp("abi")
    src, exe = d / "layout.c", d / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {key: tuple(int(v) for v in vals) for key, *vals in (line.split() for line in out.splitlines())}


def test_every_struct_layout_matches_the_header(compiled):
    """A silent mismatch would scramble kernel arguments.  The member's size is compared as well as its offset: a wrong array
    length or an int32 / int64 swap can hide behind the next field's alignment."""
    mirrors = _mirrors()
    declared = set(re.findall(r"\btypedef\s+struct\s+(\w+)", _header_code()))
    assert set(mirrors) == declared, set(mirrors) ^ declared
    assert len(mirrors) >= 29
    for name, st in mirrors.items():
        assert compiled[name] == (C.sizeof(st),), name
        for field, _ in st._fields_:
            desc = getattr(st, field)
            assert compiled[f"{name}.{field}"] == (desc.offset, desc.size), (name, field)


def test_version_macros_match_the_header(compiled):
    assert (_lib.ABI_VERSION,) == compiled["GRL_ABI_VERSION"] and _lib.ABI_VERSION >= 32
    assert (_lib.METRIC_COUNT,) == compiled["GRL_METRIC_COUNT"]


_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}


def _ctype(decl: str, is_return: bool = False):
    """One C parameter declaration (or return type) as the ctypes type the binding has to use for it."""
    if "*" in decl:
        m = re.fullmatch(r"const\s+(Grl\w+)\s*\*\s*\w*", decl)
        if m:
            return C.POINTER(getattr(_lib, m.group(1)))
        if is_return:
            assert re.fullmatch(r"const\s+char\s*\*", decl), decl
            return C.c_char_p
        return C.c_void_p
    return _SCALARS[decl.split()[0]]


def test_signature_table_matches_every_prototype():
    """Needs no built library: the table is compared, name by name and in order, with the prototypes parsed from the header."""
    protos = re.findall(r"([\w\s\*]+?)\b(grl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header_code())
    parsed = {}
    for ret, name, params in protos:
        params = [p.strip() for p in params.split(",")]
        argtypes = [] if params == ["void"] else [_ctype(p) for p in params]
        assert name not in parsed, name
        parsed[name] = (_ctype(ret.strip(), is_return=True), argtypes)
    assert list(parsed) == list(_lib.SIGNATURES) == _lib.EXPORTS and len(parsed) >= 55
    for name, sig in parsed.items():
        assert _lib.SIGNATURES[name] == sig, name
