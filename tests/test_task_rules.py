"""The rule table of the restoration tasks (task_rules.py) against what the entry points decided before there was one:
tests/golden/tasks/verdicts.json, recorded by tools/make_golden_task_verdicts.py at the commit before the table, replayed here case by
case through the same ``run_case``.  The file also pins the three places where the callers have always disagreed."""
import json
import time

import pytest

from grl_image_restoration_amd import data as D, evaluate as EV, task_rules as R
from tools import make_golden_task_verdicts as V


@pytest.fixture(scope="module")
def recorded():
    with open(V.OUT) as f:
        return json.load(f)


def test_task_lists_come_from_the_rules():
    assert tuple(R.RULES) == EV.TASKS == ("sr", "dn", "dm", "sr_bicubic", "bsr", "db", "jpeg")
    assert D.TASKS == ("sr", "sr_bicubic", "dn", "dm", "db", "jpeg") and set(D.TASKS) == {t for t, r in R.RULES.items() if r.trainable}
    assert R.SYNTHESISED == ("dn", "dm", "sr_bicubic", "db", "jpeg")
    assert all(r.cite for r in R.RULES.values())
    assert R.resolve("db", "task_inputs").sigma == 2.0 and R.resolve("sr", "evaluate", lq=True).scale == 4
    with pytest.raises(ValueError):
        R.resolve("bsr", "sampler", lq=True)


def test_verdicts_match_the_parent(recorded, tmp_path):
    cases = V.cases()
    ids = {(c["entry"], c["task"], c["label"]) for c in cases}
    assert ids == {(e, t, l) for e, ts in recorded.items() for t, ls in ts.items() for l in ls} and len(ids) == len(cases)
    env, t0, wrong = V.Env(str(tmp_path)), time.perf_counter(), []
    for c in cases:
        got, want = V.run_case(c, env), recorded[c["entry"]][c["task"]][c["label"]]
        if got != want:
            wrong.append((c["entry"], c["task"], c["label"], c["options"], got, want))
    print(f"replayed {len(cases)} cases in {time.perf_counter() - t0:.2f} s")
    assert not wrong, wrong


def test_the_grid_decides_both_ways_and_holds_the_drifts(recorded):
    good = ("accepted", "ok")
    for entry in ("evaluate.main", "train.main", "task_inputs", "PatchSampler"):
        assert set(recorded[entry]) == set(V.ENTRIES[entry])
        for task, verdicts in recorded[entry].items():
            kinds = {v.split()[0] in good for v in verdicts.values()}
            assert kinds == {True, False}, (entry, task)
            assert {v.split()[0] for v in verdicts.values()} <= {"accepted", "exit2", "ok", "ValueError", "TypeError"}, (entry, task)
    # a sigma on dm: evaluate takes and ignores it, train refuses it
    assert recorded["evaluate.main"]["dm"]["sigma_toggled"] == "accepted" and recorded["train.main"]["dm"]["sigma_toggled"] == "exit2"
    # dm at patch 2: the sampler refuses it, the train command line lets it through to the sampler
    assert recorded["PatchSampler"]["dm"]["patch_2"] == "ValueError" and recorded["train.main"]["dm"]["patch_2"].startswith("accepted")
    # an LQ folder on dm: evaluate_folder ignores what its command line refuses
    assert recorded["evaluate_folder"]["dm"]["lq_toggled"] == "ok" and recorded["evaluate.main"]["dm"]["lq_toggled"] == "exit2"
    assert recorded["train.main"]["db"]["base"] == "accepted scale=1 sigma=2.0" and recorded["train.main"]["sr"]["base"] == "accepted scale=4 sigma=None"
