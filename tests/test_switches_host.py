"""The TP_* runtime switches are declared once (csrc/tp_switches.hpp -> engine.switch_table()): the documentation lists exactly
that table, no test names a switch that does not exist, and tests/switches.py strips, checks and restores as it says.  No GPU:
the child here is a stand-in that only reports its environment."""
import glob
import os
import re

import pytest

import switches

ROOT = switches.ROOT
STAND_IN = "switches_stand_in.py"        # tests/: writes its own TP_* environment to the .npz
TYPO = "TP_" + "GRAHP"                   # (in two pieces: the test of the names in tests/*.py reads this file too)


@pytest.fixture(scope="module")
def table(hip_lib):
    from thermalporous_amd import engine
    return engine.switch_table()


def test_table_matches_the_documentation(table):
    from thermalporous_amd import engine
    names = [e["name"] for e in table]
    assert len(names) == 31 and len(set(names)) == 31 and all(n.startswith("TP_") for n in names)
    assert {e["kind"] for e in table} == {"flag", "int", "real"} and {e["when"] for e in table} == {"process", "setup"}
    assert all(e["default"] in ("0", "1") for e in table if e["kind"] == "flag") and all(e["effect"] for e in table)
    assert not set(names) & set(engine.PYTHON_SIDE_SWITCHES)
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("\n## 10. "):]
    rows = re.findall(r"^\| `(TP_[A-Z0-9_]+)` \| ([^|]*?) \|", sec, flags=re.M)
    assert sorted(r[0] for r in rows) == sorted(names + list(engine.PYTHON_SIDE_SWITCHES))
    assert len(rows) == len(set(r[0] for r in rows)) == 33
    doc = dict(rows)
    for e in table:
        assert doc[e["name"]] == e["default"], e["name"]


def test_every_switch_named_in_the_tests_exists(table):
    from thermalporous_amd import engine
    known = {e["name"] for e in table} | set(engine.PYTHON_SIDE_SWITCHES)
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))) + [os.path.join(ROOT, "bench.py")]
    seen = set()
    for f in files:
        for name in re.findall(r"[\"'](TP_[A-Z0-9_]+)[\"']", open(f).read()):       # complete quoted literals only
            assert name in known, (os.path.basename(f), name)
            seen.add(name)
    assert len(seen) > 20


def test_run_child_strips_checks_and_passes_through(table, monkeypatch, tmp_path):
    monkeypatch.setenv("TP_GRAPH", "0")
    monkeypatch.setenv("TP_LOCAL_DEVICE", "0")
    got = switches.run_child(STAND_IN, {"TP_PIN": "0"}, out=tmp_path/"env.npz", timeout=60)
    env = dict(zip(got["names"].tolist(), got["values"].tolist()))
    assert env.get("TP_PIN") == "0" and "TP_GRAPH" not in env and env.get("TP_LOCAL_DEVICE") == "0"


def test_unknown_names_and_too_many_children_start_nothing(table, monkeypatch, tmp_path):
    def no_start(*a, **k):
        raise RuntimeError("a child was started")
    monkeypatch.setattr(switches.subprocess, "Popen", no_start)
    with pytest.raises(AssertionError, match=TYPO):
        switches.run_child(STAND_IN, {TYPO: "0"}, out=tmp_path/"a.npz")
    with pytest.raises(AssertionError, match=TYPO):
        switches.run_children(STAND_IN, {"a": {}, "b": {TYPO: "0"}}, tmp_path)
    with pytest.raises(AssertionError, match="at most 4"):
        switches.run_children(STAND_IN, {str(i): {} for i in range(5)}, tmp_path)
    with pytest.raises(RuntimeError):                       # (the guard itself: four valid settings would start)
        switches.run_children(STAND_IN, {str(i): {} for i in range(4)}, tmp_path)


def test_setup_env_takes_per_setup_switches_only(table, monkeypatch):
    with pytest.raises(AssertionError, match="once per process"):
        with switches.setup_env(TP_GRAPH="0"):
            pass
    with pytest.raises(AssertionError, match=TYPO):
        with switches.setup_env(**{TYPO: "0"}):
            pass
    for before in (None, "512"):
        if before is None:
            monkeypatch.delenv("TP_AMG_TAIL_CELLS", raising=False)
        else:
            monkeypatch.setenv("TP_AMG_TAIL_CELLS", before)
        with switches.setup_env(TP_AMG_TAIL_CELLS="8"):
            assert os.environ["TP_AMG_TAIL_CELLS"] == "8"
        assert os.environ.get("TP_AMG_TAIL_CELLS") == before
