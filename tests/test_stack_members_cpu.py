"""The `surrogate_stacks:` key of rollout_surrogates (driver.stack_config) and who refuses what: no GPU."""
import numpy as np
import pytest

from test_mlp_stack_cpu import a_stack


def config(tmp_path, models=("single",), stacks=("deep",), committees=None, **more):
    """A loaded configuration with fixed models (files of the 5 -> 10 -> 4 shape) and stacks written by write_surrogate_stack."""
    from miniweatherml_amd import mlp
    np.savetxt(tmp_path / "w.txt", np.zeros(104))
    np.savetxt(tmp_path / "si.txt", np.array([[0., 1.]] * 5))
    np.savetxt(tmp_path / "so.txt", np.array([[0., 1.]] * 4))
    fixed = {"keras_weights_txt": str(tmp_path / "w.txt"), "nn_input_scaling": str(tmp_path / "si.txt"), "nn_output_scaling": str(tmp_path / "so.txt")}
    w, si, so = mlp.write_surrogate_stack(a_stack("tendency", 9), str(tmp_path / "stack"))
    cfg = {"_dir": str(tmp_path), "surrogate_stacks": [{"name": n, "keras_weights_txt": w, "nn_input_scaling": si, "nn_output_scaling": so} for n in stacks]}
    if models:
        cfg["surrogate_models"] = [dict(fixed, name=n) for n in models]
    if committees:
        cfg["surrogate_committees"] = committees
    return dict(cfg, **more), fixed


def test_member_count_follows_from_the_three_lists(tmp_path):
    from miniweatherml_amd import driver
    cfg, _ = config(tmp_path, models=("a", "b"), stacks=("deep", "wide"), committees=[{"name": "both", "members": ["a", "b"]}])
    assert [s["name"] for s in driver.stack_config(cfg)] == ["deep", "wide"]
    assert driver.rollout_config(cfg)[3] == 1 + 2 + 1 + 2 + 1
    assert driver.rollout_config(dict(cfg, persistence_member=False))[3] == 6
    with pytest.raises(ValueError, match="2 surrogate_stacks.*are 7 members"):
        driver.rollout_config(dict(cfg, nens=5, _nens_given=True))


def test_stacks_alone_are_a_rollout(tmp_path):
    from miniweatherml_amd import driver
    cfg, _ = config(tmp_path, models=())
    models, interval, persistence, nens = driver.rollout_config(cfg)
    assert (models, interval, persistence, nens) == ([], 1, True, 3)
    assert driver.harvest_config(dict(cfg, harvest={"seed": 1}))["members"] == ["deep"]
    with pytest.raises(KeyError, match="surrogate_models"):
        driver.rollout_config({"_dir": str(tmp_path)})


@pytest.mark.parametrize("case", ["model", "committee", "twice", "kessler", "fixed file", "committee member", "outside"])
def test_refusals_name_the_entry(tmp_path, case):
    from miniweatherml_amd import driver
    both = [{"name": "both", "members": ["single"]}]
    if case == "fixed file":
        cfg, fixed = config(tmp_path)
        cfg["surrogate_stacks"] = [dict(fixed, name="plain")]
    else:
        cfg, _ = config(tmp_path, stacks={"model": ("single",), "committee": ("both",), "twice": ("deep", "deep"), "kessler": ("kessler",)}.get(case, ("deep",)),
                        committees=[{"name": "both", "members": ["single", "deep"]}] if case == "committee member" else both)
    if case == "outside":
        cfg["harvest"] = {"outside": True}
    match = {"model": "'single' has the name", "committee": "'both' has the name", "twice": "'deep' has the name", "kessler": "'kessler' and 'persistence'",
             "fixed file": "'plain'.*no `# stack:` header", "committee member": "'both' names 'deep', which is a stack", "outside": "stack member.*'deep'"}[case]
    with pytest.raises(ValueError, match=match):
        driver.harvest_config(cfg) if case == "outside" else driver.stack_config(cfg)


def test_surrogate_models_still_refuse_a_stack_file(tmp_path):
    from miniweatherml_amd import driver
    cfg, _ = config(tmp_path)
    with pytest.raises(ValueError, match="surrogate_stacks.*inference_ponni only"):
        driver._surrogate_models([dict(cfg["surrogate_stacks"][0], name="wide")], str(tmp_path))
