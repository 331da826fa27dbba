"""The driver's experiment classes without a GPU and without the library: the order of the calls a step makes, on recording stubs in
place of the coupler, the dycore, the microphysics and the scorers, and the keys of the two JSON documents."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

from miniweatherml_amd import driver, experiments


class Rec:
    """A stub whose every method appends (its name, the method, the arguments worth keeping) to one shared log."""

    def __init__(self, log, name, **attrs):
        self.log, self.name = log, name
        self.__dict__.update(attrs)

    def __getattr__(self, method):
        def call(*args, **kw):
            self.log.append((self.name + "." + method,) + tuple(a for a in args if isinstance(a, (int, float, str))))
        return call


@pytest.fixture
def log(monkeypatch):
    """The shared log, with the free functions and the input copy of a step recorded in it too."""
    out = []
    for mod in (driver.column, experiments):
        monkeypatch.setattr(mod, "sponge_layer", lambda coupler, dt, *scale: out.append(("sponge_layer", dt) + scale))
    monkeypatch.setattr(driver, "Coupler", lambda device: Rec(out, "inp"))
    return out


def bound(cls, log, cfg=None, **attrs):
    """An experiment of class cls as setup leaves it, with stubs for its collaborators."""
    exp = cls()
    exp.cfg, exp.info, exp.device, exp.quiet, exp.nstep = cfg or {}, {"experiment": "x"}, "cpu", True, 0
    exp.coupler, exp.dycore, exp.micro, exp.nudger = (Rec(log, n) for n in ("coupler", "dycore", "micro", "nudger"))
    exp.__dict__.update(attrs)
    return exp


def march(exp, n, dt=0.5):
    for k in range(n):
        exp.step(dt, k * dt)


def test_every_experiment_has_its_class():
    assert tuple(driver.EXPERIMENT_CLASSES) == driver.EXPERIMENTS
    assert [n for n, c in driver.EXPERIMENT_CLASSES.items() if c.timed] == ["community_benchmark"]


def test_column_order(log):
    exp = bound(driver.EXPERIMENT_CLASSES["supercell_example"], log)
    march(exp, 2)
    one = [("dycore.time_step", 0.5), ("micro.time_step", 0.5), ("sponge_layer", 0.5), ("nudger.nudge_to_column", 0.5)]
    assert log == one + one and exp.nstep == 2


def test_city_order(log):
    exp = bound(driver.SimpleCity, log, horiz_sponge=Rec(log, "horiz_sponge"), time_averager=Rec(log, "averager"))
    march(exp, 1)
    assert log == [("horiz_sponge.apply", 0.5, True, True, False, False), ("dycore.time_step", 0.5), ("sponge_layer", 0.5, 1),
                   ("averager.accumulate", 0.5)]
    exp.finish(1, "in.yaml")
    assert log[-1] == ("averager.finalize",)


def test_statistics_and_samples_keep_the_input(log):
    exp = bound(driver.GatherStatistics, log, stats=Rec(log, "stats"))
    march(exp, 1)
    assert log[:5] == [("dycore.time_step", 0.5), ("coupler.clone_into",), ("micro.time_step", 0.5),
                       ("stats.gather_micro_statistics", 0.5, 0.0), ("sponge_layer", 0.5)]
    del log[:]
    gen = SimpleNamespace(generate_samples_stencil=lambda inp, coupler, dt, etime: log.append(("generate", inp.name, dt, etime)) or 7)
    exp = bound(driver.GenerateMicroData, log, datagen=gen)
    exp.info["samples"] = 0
    march(exp, 2)
    assert log[1:4] == [("coupler.clone_into",), ("micro.time_step", 0.5), ("generate", "inp", 0.5, 0.0)] and exp.info["samples"] == 14


def test_evaluation_steps(log):
    exp = bound(driver.EvaluateSurrogates, log, {"eval_interval": 2}, evaluator=Rec(log, "evaluator"), domain_eval=Rec(log, "domain"),
                committee_evals=[({"name": "c"}, Rec(log, "committee"))], eval_calls=[])
    march(exp, 4)
    plain = [("dycore.time_step", 0.5), ("micro.time_step", 0.5), ("sponge_layer", 0.5), ("nudger.nudge_to_column", 0.5)]
    scored = [("dycore.time_step", 0.5), ("coupler.clone_into",), ("micro.time_step", 0.5), ("evaluator.accumulate",), ("domain.accumulate",),
              ("committee.accumulate",), ("sponge_layer", 0.5), ("nudger.nudge_to_column", 0.5)]
    assert log == scored + plain + scored + plain
    assert exp.eval_calls == [{"step": 0, "etime": 0.0}, {"step": 2, "etime": 1.0}] and exp.nstep == 4


def test_rollout_steps(log):
    flags = []
    micro = Rec(log, "micro")
    micro.time_step = lambda coupler, dt: flags.append((micro.harvest_now, micro.harvest_etime, micro.domain_now))
    exp = bound(driver.RolloutSurrogates, log, {"eval_interval": 2}, harvest={"interval": 3}, harvester=object(), domain_cfg={"margin": 0.0},
                scorer=Rec(log, "scorer", diverged_at={}), rain=Rec(log, "rain"), micro=micro)
    march(exp, 6)
    assert [f[0] for f in flags] == [True, False, False, True, False, False]
    assert [f[1] for f in flags] == [0.0, 0.5, 1.0, 1.5, 2.0, 2.5]
    assert [f[2] for f in flags] == [True, False, True, False, True, False]
    want = []
    for k in range(6):
        want += [("dycore.time_step", 0.5), ("sponge_layer", 0.5), ("nudger.nudge_to_column", 0.5)]
        if k % 2 == 0:
            want += [("scorer.accumulate", k, 0.5 * k + 0.5), ("micro.guard_record", k, 0.5), ("micro.domain_record", k),
                     ("rain.accumulate", k, 0.5 * k + 0.5)]
    assert log == want and exp.nstep == 6


def test_rollout_reports_a_member_that_diverges_once(log, capsys):
    scorer = Rec(log, "scorer", diverged_at={"a": None, "b": {"step": 0}})
    scorer.accumulate = lambda coupler, step, etime: scorer.diverged_at.update(a={"step": step})
    exp = bound(driver.RolloutSurrogates, log, {"eval_interval": 1}, harvester=None, domain_cfg=None, scorer=scorer, rain=None, quiet=False)
    march(exp, 2)
    assert capsys.readouterr().out == "rollout_surrogates: member 'a' is non-finite at step 0\n"


EVAL_KEYS = ["experiment", "yaml", "eval_interval", "steps", "models", "statistics", "fields", "classes", "report", "history"]


def test_evaluation_document():
    banks = [SimpleNamespace(models=2, n_in=5, forms=["state", "tendency"], domain_group=4), SimpleNamespace(models=1, n_in=9, forms=["state"], domain_group=2)]
    evaluator = SimpleNamespace(banks=banks, history=[["h0a", "h0b"], ["h2a", "h2b"]])
    models = [{"name": "a"}, {"name": "b"}, {"name": "s"}]
    calls = [{"step": 0, "etime": 0.0}, {"step": 2, "etime": 1.0}]
    doc = driver.evaluation_document("evaluate_surrogates", "in.yaml", 2, 4, evaluator, models, calls, {"a": 1})
    assert list(doc) == EVAL_KEYS and doc["yaml"] == driver.os.path.abspath("in.yaml") and (doc["eval_interval"], doc["steps"]) == (2, 4)
    assert doc["models"] == [{"name": "a", "bank": 0, "n_in": 5, "form": "state"}, {"name": "b", "bank": 0, "n_in": 5, "form": "tendency"},
                             {"name": "s", "bank": 1, "n_in": 9, "form": "state"}]
    assert doc["report"] == {"a": 1} and doc["history"] == [{"step": 0, "etime": 0.0, "banks": ["h0a", "h0b"]}, {"step": 2, "etime": 1.0, "banks": ["h2a", "h2b"]}]
    ce = SimpleNamespace(bank=banks[0], history=["ch"], report=lambda: {"mean": 1})
    domain_eval = SimpleNamespace(names=["a", "b", "s"], boxes=np.zeros((3, 5, 2)), history=[["d0"], ["d2"]])
    eval_domain = {"margin": 0.0, "fields": ["temp"], "box_of": None}
    full = driver.evaluation_document("evaluate_surrogates", "in.yaml", 2, 4, evaluator, models, calls, {"a": 1},
                                      [({"name": "c", "members": ["b", "a"]}, ce)], eval_domain, domain_eval, {"a": {"inside": 1}})
    assert list(full) == EVAL_KEYS + ["committees", "domain"]
    assert list(full["committees"][0]) == ["name", "members", "n_in", "statistics", "report", "history"] and full["committees"][0]["report"] == {"mean": 1}
    assert list(full["domain"]) == ["margin", "fields", "box_of", "group", "models", "history"] and full["domain"]["group"] == {"5": 4, "9": 2}
    assert list(full["domain"]["models"]) == ["a", "b", "s"] and full["domain"]["models"]["a"]["report"] == {"inside": 1}
    assert full["domain"]["models"]["b"] == {"box": driver.surrogate_eval.box_json(np.zeros((5, 2))), "report": {}}
    assert full["domain"]["history"] == [{"step": 0, "etime": 0.0, "banks": ["d0"]}, {"step": 2, "etime": 1.0, "banks": ["d2"]}]
    json.dumps(full)
    empty = driver.evaluation_document("evaluate_surrogates", "in.yaml", 2, 0, SimpleNamespace(banks=banks, history=[]), models, [], {},
                                       [({"name": "c", "members": ["b", "a"]}, ce)])
    assert empty["committees"][0]["report"] == {} and empty["history"] == [] and "domain" not in empty


ROLLOUT_KEYS = ["experiment", "yaml", "eval_interval", "steps", "members", "models", "fields", "statistics", "history", "report", "diverged_at"]


def test_rollout_document():
    scorer = SimpleNamespace(member_names=["kessler", "a", "b", "plain", "guarded", "persistence"], fields=("temp",), history=[[1.0]])
    micro = SimpleNamespace(model_forms=["state", "tendency"], guard_reports=lambda: [None, {"columns": 4}])
    models = [{"name": "a"}, {"name": "b"}]
    rep = {"times": [{"step": 0}], "diverged_at": {"a": None}}
    doc = driver.rollout_document("rollout_surrogates", "in.yaml", 2, 4, models, scorer, rep, micro)
    assert list(doc) == ROLLOUT_KEYS and doc["members"] == scorer.member_names and doc["statistics"] == list(driver.rollout.ROLLOUT_STATS)
    assert doc["models"] == [{"name": "a", "member": 1, "form": "state"}, {"name": "b", "member": 2, "form": "tendency"}]
    assert doc["report"] == rep["times"] and doc["diverged_at"] == {"a": None} and doc["history"] == [[1.0]]
    json.dumps(doc, allow_nan=False)
    committees = [{"name": "plain", "members": ["a", "b"]}, {"name": "guarded", "members": ["a", "b"], "guard": {"temp": 1.0}}]
    blocks = [None, {"cells": 1}, {"cells": 2}, {"cells": 3}, {"cells": 4}, None]
    rain = SimpleNamespace(times=[{"step": 0}])
    full = driver.rollout_document("rollout_surrogates", "in.yaml", 2, 4, models, scorer, rep, micro, committees, domain_blocks=blocks,
                                   harvest={"interval": 2, "calls": 2}, rain_cfg={"thresholds_mm": [1.0], "map": False}, rain=rain)
    assert list(full) == ROLLOUT_KEYS + ["committees", "harvest", "surface_rain"]
    assert full["committees"] == [{"name": "plain", "members": ["a", "b"], "member": 3, "domain": {"cells": 3}},
                                  {"name": "guarded", "members": ["a", "b"], "guard": {"columns": 4}, "member": 4, "domain": {"cells": 4}}]
    assert list(full["committees"][1]) == ["name", "members", "guard", "member", "domain"]
    assert [m["domain"] for m in full["models"]] == [{"cells": 1}, {"cells": 2}] and list(full["models"][0]) == ["name", "member", "form", "domain"]
    assert full["harvest"] == {"interval": 2, "calls": 2} and full["surface_rain"] == {"thresholds_mm": [1.0], "map": False, "report": [{"step": 0}]}
    assert "guard" not in committees[0] and committees[1]["guard"] == {"temp": 1.0} and "domain" not in models[0]          # the inputs are left alone
    json.dumps(full, allow_nan=False)
    for only, added in (({"committees": committees}, ["committees"]), ({"domain_blocks": blocks}, []), ({"harvest": {"calls": 0}}, ["harvest"]),
                        ({"rain_cfg": {"map": True}, "rain": rain}, ["surface_rain"])):                # each optional block alone
        one = driver.rollout_document("rollout_surrogates", "in.yaml", 2, 4, models, scorer, rep, micro, **only)
        assert list(one) == ROLLOUT_KEYS + added and ("domain" in one["models"][0]) == ("domain_blocks" in only)
