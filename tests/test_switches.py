"""The GRL_* environment switches have one definition (grl_image_restoration_amd/switches.py): the sources read exactly the switches
the table declares, DESIGN.md's "Knobs" section lists exactly those, the accessors parse as the hand-written expressions they replaced,
and an undeclared or C-side name cannot be read from Python.  The same rule at compile time: csrc has one build.  No GPU, no
library: sources, the document and os.environ only."""
import glob
import os
import re

import pytest

from grl_image_restoration_amd import metrics
from grl_image_restoration_amd import switches as SW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "grl_image_restoration_amd")
NAME = r'"(GRL_[A-Z0-9_]+)"'
BOOLS = [s for s in SW.TABLE.values() if s.where == "py" and s.kind in ("on", "off")]
NUMS = [s for s in SW.TABLE.values() if s.where == "py" and s.kind in ("int", "float")]


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def test_sources_read_exactly_the_declared_switches():
    py, direct = set(), {}
    for path in glob.glob(os.path.join(PKG, "*.py")):
        src = _read(path)
        py |= set(re.findall(r"\bSW\.(?:on|num|text|is_set)\(\s*" + NAME, src))
        if re.search(r"\bSW\.text\(NIQE_ENV\b", src):            # metrics.py reads its switch through the constant it exports
            py.add(metrics.NIQE_ENV)
        direct[os.path.basename(path)] = set(re.findall(r"(?:environ|getenv)[^\n]*?" + NAME, src))
    assert {k for k, v in direct.items() if v} <= {"switches.py"}, f"GRL_* read outside the accessors: {direct}"
    csrc = set()
    for path in glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.h")):
        csrc |= set(re.findall(r"\b(?:getenv|grl_env_int)\(\s*" + NAME, _read(path)))
    assert py == {n for n, s in SW.TABLE.items() if s.where == "py"}
    assert csrc == {n for n, s in SW.TABLE.items() if s.where == "csrc"}
    assert all(n == s.name and s.kind in ("on", "off", "int", "float", "str") and s.when in ("import", "plan", "call") and s.doc
               for n, s in SW.TABLE.items())


def test_csrc_has_one_build():
    """No compile-time toggle either: the only preprocessor conditionals of csrc test the compiler's own __HIPCC__, and the
    Makefile defines nothing."""
    paths = glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.h"))
    assert paths
    toggles = []
    for path in paths:
        for n, line in enumerate(_read(path).split("\n"), 1):
            m = re.match(r"\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)", line)
            if m and set(re.findall(r"[A-Za-z_]\w*", m.group(1).split("//")[0])) - {"defined"} != {"__HIPCC__"}:
                toggles.append(f"{os.path.basename(path)}:{n}: {line.strip()}")
    assert not toggles, toggles
    defines = [w for w in _read(os.path.join(PKG, "csrc", "Makefile")).split() if w.startswith("-D")]
    assert not defines, defines


def test_design_knobs_section_lists_exactly_the_declared_switches():
    design = _read(os.path.join(ROOT, "DESIGN.md"))
    start = design.index("### Knobs")
    knobs = design[start:design.index("\n## ", start)]
    assert set(re.findall(r"GRL_[A-Z0-9_]+", knobs)) == set(SW.TABLE)
    for doc in ("README.md", "INTEGRATION.md"):       # the shorter documents may name a switch only if it exists
        named = set(re.findall(r"`(GRL_[A-Z0-9_]+)(?:=[^`]*)?`", _read(os.path.join(ROOT, doc))))
        stale = {n for n in named - set(SW.TABLE) if not n.startswith(("GRL_EPI_", "GRL_ERR_", "GRL_DT_", "GRL_METRIC_"))}   # C enums
        assert not stale, (doc, stale)


@pytest.mark.parametrize("value", [None, "", "0", "1", "2", "true"])
def test_boolean_parsing_is_the_old_expression(monkeypatch, value):
    assert BOOLS
    for s in BOOLS:
        if value is None:
            monkeypatch.delenv(s.name, raising=False)
        else:
            monkeypatch.setenv(s.name, value)
        old = os.environ.get(s.name, "1") != "0" if s.kind == "on" else os.environ.get(s.name, "0") == "1"
        assert SW.on(s.name) is old, (s.name, value)
        assert SW.is_set(s.name) is (value is not None)
        assert s.default is (s.kind == "on")


def test_numeric_parsing(monkeypatch):
    assert NUMS
    for s in NUMS:
        kind = int if s.kind == "int" else float
        monkeypatch.delenv(s.name, raising=False)
        if s.default is SW.SITE:
            with pytest.raises(TypeError):
                SW.num(s.name)
            assert SW.num(s.name, default=5) == 5
        else:
            got = SW.num(s.name)
            assert got == s.default and type(got) is kind
        monkeypatch.setenv(s.name, "7")
        got = SW.num(s.name, default=5)
        assert got == 7 and type(got) is kind


def test_text_switches(monkeypatch):
    monkeypatch.delenv("GRL_PRECISION", raising=False)
    monkeypatch.delenv("GRL_HIGH_CAB", raising=False)
    assert SW.text("GRL_PRECISION", default="auto") == "auto" and SW.text("GRL_HIGH_CAB") == ""
    monkeypatch.setenv("GRL_PRECISION", "high")
    assert SW.text("GRL_PRECISION", default="auto") == "high"
    assert metrics.NIQE_ENV == "GRL_NIQE_PARAMS" and SW.TABLE[metrics.NIQE_ENV].kind == "str"


def test_misuse_fails():
    csrc = [n for n, s in SW.TABLE.items() if s.where == "csrc"]
    assert "GRL_PERSIST_GRID" in csrc
    for fn in (SW.on, SW.num, SW.text, SW.is_set):
        with pytest.raises(KeyError):
            fn("GRL_NOT_A_SWITCH")
        for n in csrc:
            with pytest.raises(ValueError):
                fn(n)
    with pytest.raises(TypeError):
        SW.on("GRL_SPLIT_STREAMS")            # an int switch is not a boolean
    with pytest.raises(TypeError):
        SW.num("GRL_CALIBRATE")
