"""The `surrogate_stacks:` key of evaluate_surrogates: what the configuration accepts and refuses, and the `stacks`
block of surrogate_evaluation.json.  No GPU."""
from types import SimpleNamespace

import pytest

from test_stack_members_cpu import config


def configured(cfg):
    from miniweatherml_amd import driver
    exp = driver.EvaluateSurrogates()
    exp.configure(cfg, 1)
    return exp


def test_stacks_alone_are_an_evaluation(tmp_path):
    cfg, _ = config(tmp_path, models=(), stacks=("deep", "wide"), eval_interval=3)
    exp = configured(cfg)
    assert [s["name"] for s in exp.stacks] == ["deep", "wide"] and cfg["surrogate_models"] == [] and cfg["eval_interval"] == 3
    with pytest.raises(ValueError, match="eval_domain.*surrogate_stacks only"):
        configured(dict(config(tmp_path, models=())[0], eval_domain=True))


def test_without_the_key_nothing_changes(tmp_path):
    cfg, _ = config(tmp_path, models=("a", "b"))
    del cfg["surrogate_stacks"]
    exp = configured(cfg)
    assert exp.stacks == [] and [m["name"] for m in cfg["surrogate_models"]] == ["a", "b"] and exp.eval_domain is None
    with pytest.raises(KeyError, match="surrogate_models"):
        configured({"_dir": str(tmp_path)})


def test_refusals_name_the_stack(tmp_path):
    cfg, _ = config(tmp_path, stacks=["s%d" % k for k in range(33)])
    with pytest.raises(ValueError, match="at most 32 surrogate_stacks.*'s32'"):
        configured(cfg)
    cfg, _ = config(tmp_path, eval_domain={"box_of": "deep"})
    with pytest.raises(ValueError, match="box_of names 'deep', which is a stack"):
        configured(cfg)
    assert configured(dict(cfg, eval_domain={"box_of": "single"})).eval_domain["box_of"] == "single"


def test_evaluation_document_lists_the_stacks():
    from miniweatherml_amd import driver
    fixed = SimpleNamespace(models=1, n_in=5, forms=["state"], domain_group=4)
    group = SimpleNamespace(models=2, n_ins=[9, 5], forms=["tendency", "state"], widths=[[9, 17, 5, 4], [5, 32, 4]],
                            stacks=[SimpleNamespace(slopes=[0.5, 0.25]), SimpleNamespace(slopes=[0.125])])
    evaluator = SimpleNamespace(banks=[fixed, group], history=[["h0", "g0"]])
    stacks = [{"name": "deep", "keras_weights_txt": "w"}, {"name": "wide", "keras_weights_txt": "v"}]
    domain_eval = SimpleNamespace(names=["a"], boxes=[[[0.0, 1.0]] * 5], history=[["d0"]])
    doc = driver.evaluation_document("evaluate_surrogates", "in.yaml", 1, 1, evaluator, [{"name": "a"}], [{"step": 0, "etime": 0.0}], {},
                                     eval_domain={"margin": 0.0, "fields": ["temp"], "box_of": None}, domain_eval=domain_eval, drep={}, stacks=stacks)
    assert doc["models"] == [{"name": "a", "bank": 0, "n_in": 5, "form": "state"}] and doc["history"][0]["banks"] == ["h0", "g0"]
    assert doc["stacks"] == [{"name": "deep", "keras_weights_txt": "w", "bank": 1, "widths": [9, 17, 5, 4], "slopes": [0.5, 0.25], "form": "tendency"},
                             {"name": "wide", "keras_weights_txt": "v", "bank": 1, "widths": [5, 32, 4], "slopes": [0.125], "form": "state"}]
    assert doc["domain"]["group"] == {"5": 4} and list(doc["domain"]["models"]) == ["a"]
    alone = driver.evaluation_document("evaluate_surrogates", "in.yaml", 1, 0, SimpleNamespace(banks=[group], history=[]), [], [], {}, stacks=stacks)
    assert alone["models"] == [] and [s["bank"] for s in alone["stacks"]] == [0, 0]
