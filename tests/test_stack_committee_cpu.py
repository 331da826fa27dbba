"""`surrogate_committees:` entries that name stacks of `surrogate_stacks:` (driver.committee_config): no GPU."""
import pytest

from test_mlp_stack_cpu import a_stack
from test_stack_members_cpu import config

BOTH = [{"name": "both", "members": ["deep", "wide"]}]


@pytest.mark.parametrize("models", [("single",), ()])
def test_a_committee_of_stacks_is_accepted_and_counted(tmp_path, models):
    from miniweatherml_amd import driver
    cfg, _ = config(tmp_path, models=models, stacks=("deep", "wide"), committees=BOTH)
    assert driver.committee_config(cfg) == [{"name": "both", "members": ["deep", "wide"], "stacks": True}]
    assert driver.rollout_config(cfg)[3] == 1 + len(models) + 1 + 2 + 1
    assert [s["name"] for s in driver.stack_config(cfg)] == ["deep", "wide"]


@pytest.mark.parametrize("case", ["model+stack", "n_in", "guard", "twice", "17", "harvest", "training_domain", "inference_ponni"])
def test_refusals_name_the_committee(tmp_path, case):
    from miniweatherml_amd import driver, mlp
    names = tuple("s%d" % k for k in range(17)) if case == "17" else ("deep", "wide")
    members = {"model+stack": ["single", "deep"], "twice": ["deep", "deep"], "17": list(names)}.get(case, ["deep", "wide"])
    cfg, _ = config(tmp_path, stacks=names, committees=[dict({"name": "both", "members": members}, **({"guard": {"temp": 1.0}} if case == "guard" else {}))])
    if case == "n_in":
        w, si, so = mlp.write_surrogate_stack(a_stack("state", 5), str(tmp_path / "five"))
        cfg["surrogate_stacks"][1].update(keras_weights_txt=w, nn_input_scaling=si, nn_output_scaling=so)
    match = {"model+stack": "committee 'both' names 'deep', which is a stack", "n_in": "'both' mixes stacks of n_in 5 and 9", "guard": "'both'.*has a guard",
             "twice": "'both' names a model twice", "17": "'both' has 17 models", "harvest": "'both', which is a committee",
             "training_domain": "training_domain.*'both'", "inference_ponni": "inference_ponni.*'both'"}[case]
    with pytest.raises(ValueError, match=match):
        if case == "harvest":
            driver.harvest_config(dict(cfg, harvest={"members": ["both"]}))
        elif case == "training_domain":
            driver.RolloutSurrogates().configure(dict(cfg, training_domain=True), 1)
        elif case == "inference_ponni":
            driver.InferencePonni().configure(cfg, 1)
        else:
            driver.committee_config(cfg)


def test_without_a_committee_of_stacks_nothing_changes(tmp_path):
    from miniweatherml_amd import driver
    cfg, _ = config(tmp_path, models=("a", "b"), committees=[{"name": "ab", "members": ["b", "a"], "guard": {"temp": 2.0, "max_rainsplit": 4}}])
    got = driver.committee_config(cfg)
    assert [{k: c[k] for k in ("name", "members")} for c in got] == [{"name": "ab", "members": ["b", "a"]}] and set(got[0]) == {"name", "members", "guard"}
    assert got[0]["guard"]["temp"] == 2.0 and driver.rollout_config(cfg)[3] == 1 + 2 + 1 + 1 + 1
    with pytest.raises(ValueError, match="'ab' names 'c', which is no surrogate model"):
        driver.committee_config(dict(cfg, surrogate_committees=[{"name": "ab", "members": ["c"]}]))
    with pytest.raises(KeyError, match="surrogate_models"):
        driver.committee_config({"_dir": str(tmp_path), "surrogate_committees": BOTH})
