"""The surrogate rollout without a GPU: the experiment's configuration (the derived member count and what it refuses), the C ABI's table,
the loud failure of the new device entry points, and the arithmetic of rollout_report / RolloutScorer on hand-made raw arrays."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entry -> number of arguments in include/mw_cdna4.h
NEW = {"mw_member_extract": 7, "mw_member_insert": 7, "mw_surrogate_members_apply": 7, "mw_member_divergence_workspace_bytes": 3,
       "mw_member_divergence": 8}
BASE = "sim_time: 10\nnx_glob: 8\nny_glob: 8\nnz: 8\nxlen: 1\nylen: 1\nzlen: 1\ndt_phys: 0\nout_prefix: x\ninit_data: supercell\nout_freq: -1\n"


def model_list(tmp_path, k):
    """k single-cell models as files: (the YAML text of their surrogate_models list, the entries surrogate_config returns)."""
    from miniweatherml_amd import modules, surrogate_train as st
    W1, b1, W2, b2, si, so = modules.load_surrogate_weights()
    w = st.initial_weights(0, k)
    _, models = st.write_outputs(str(tmp_path / "t"), w[0], si, so, {}, all_weights=w)
    return "surrogate_models:\n" + "".join("  - {%s}\n" % ", ".join('%s: "%s"' % kv for kv in m.items()) for m in models), models


def test_experiment_is_registered():
    from miniweatherml_amd import driver
    assert "rollout_surrogates" in driver.EXPERIMENTS
    assert "rollout_surrogates" in driver.__doc__


def test_member_count_is_derived_from_the_list(mw, tmp_path):
    from miniweatherml_amd import driver
    lst, models = model_list(tmp_path, 3)
    p = tmp_path / "in.yaml"
    p.write_text(BASE + lst)
    assert driver.rollout_config(driver.load_config(str(p))) == (models, 1, True, 5)          # Kessler + 3 + persistence
    p.write_text(BASE + lst + "persistence_member: false\neval_interval: 4\n")
    assert driver.rollout_config(driver.load_config(str(p))) == (models, 4, False, 4)
    p.write_text(BASE + lst + "nens: 5\n")                                                     # an agreeing nens is accepted
    assert driver.rollout_config(driver.load_config(str(p)))[3] == 5
    for bad in ("nens: 4\n", "nens: 1\n", "persistence_member: false\nnens: 5\n"):
        p.write_text(BASE + lst + bad)
        with pytest.raises(ValueError, match="leave nens out"):
            driver.rollout_config(driver.load_config(str(p)))
    p.write_text(BASE + lst + "persistence_member: 2\n")
    with pytest.raises(ValueError, match="true or false"):
        driver.rollout_config(driver.load_config(str(p)))


def test_bad_model_lists_are_refused(mw, tmp_path):
    from miniweatherml_amd import driver
    lst, models = model_list(tmp_path, 2)
    p = tmp_path / "in.yaml"
    p.write_text(BASE)
    with pytest.raises(KeyError, match="surrogate_models"):
        driver.rollout_config(driver.load_config(str(p)))
    p.write_text(BASE + "surrogate_models: []\n")
    with pytest.raises(ValueError, match="non-empty"):
        driver.rollout_config(driver.load_config(str(p)))
    p.write_text(BASE + "surrogate_models: 3\n")
    with pytest.raises(ValueError, match="non-empty list"):
        driver.rollout_config(driver.load_config(str(p)))
    p.write_text(BASE + "surrogate_models:\n  - [1, 2]\n")
    with pytest.raises(KeyError, match="name"):
        driver.rollout_config(driver.load_config(str(p)))
    p.write_text(BASE + lst.replace("weights_1.txt", "nothing.txt"))
    with pytest.raises(FileNotFoundError):
        driver.rollout_config(driver.load_config(str(p)))
    p.write_text(BASE + lst.replace("model_1", "kessler"))
    with pytest.raises(ValueError, match="members of their own"):
        driver.rollout_config(driver.load_config(str(p)))


def test_more_models_than_the_dycore_steps_members(mw, tmp_path):
    """30 members is the dycore's limit: 28 models + Kessler + persistence fit, 29 do not (29 do without the persistence member)."""
    from miniweatherml_amd import capi, driver, modules
    assert capi.MW_ROLLOUT_MAX_MEMBERS == 30
    lst, models = model_list(tmp_path, 29)
    p = tmp_path / "in.yaml"
    p.write_text(BASE + lst)
    with pytest.raises(ValueError, match="at most 30"):
        driver.rollout_config(driver.load_config(str(p)))
    p.write_text(BASE + lst + "persistence_member: false\n")
    assert driver.rollout_config(driver.load_config(str(p)))[3] == 30
    assert len(modules.rollout_member_names(["m%d" % k for k in range(28)])) == 30
    with pytest.raises(capi.MWError, match="at most 30"):
        modules.rollout_member_names(["m%d" % k for k in range(29)])
    with pytest.raises(capi.MWError, match="unique"):
        modules.rollout_member_names(["a", "a"])
    assert modules.rollout_member_names([]) == ["kessler", "persistence"]                     # (the driver refuses an empty list, the module need not)
    assert modules.rollout_member_names(["a", "b"], persistence=False) == ["kessler", "a", "b"]


def test_header_binding_table_and_exports_agree(mw):
    from miniweatherml_amd import capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mw_cdna4.h")).read(), flags=re.S)
    L = C.CDLL(capi.LIB_PATH)
    for name, nargs in NEW.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert name in capi.SYMBOLS and hasattr(L, name), name
        assert len(capi.SYMBOLS[name][1]) == nargs, name
    assert int(re.search(r"#define MW_ROLLOUT_MAX_MEMBERS (\d+)", header).group(1)) == capi.MW_ROLLOUT_MAX_MEMBERS


def test_kernels_are_in_the_library_once_and_no_dispatcher_family(mw):
    import conftest
    from miniweatherml_amd import capi
    names = set()
    for m in re.finditer(rb"_ZN2mw(\d+)([0-9A-Za-z_]+)\.kd\x00", open(capi.LIB_PATH, "rb").read()):
        names.add(m.group(2)[:int(m.group(1))].decode())
    new = {"k_members_apply", "k_members_apply_stencil", "k_members_apply_strict", "k_member_copy", "k_member_divergence",
           "k_member_divergence_final"}
    assert new <= names and not (new & conftest._DISPATCHED)


def test_entry_points_check_arguments_then_fail_loudly_without_gpu(mw):
    import torch
    from miniweatherml_amd import capi
    L = capi.lib()
    p16 = (C.c_void_p * 16)(*([0x1000] * 16))
    one = C.c_void_p(0x1000)
    members = (C.c_int * 2)(1, 2)
    assert L.mw_member_extract(0, 2, 0, 1, p16, p16, None) != 0 and b"n and nens" in L.mw_last_error()
    assert L.mw_member_extract(4, 2, 2, 1, p16, p16, None) != 0 and b"outside [0, 2)" in L.mw_last_error()
    assert L.mw_member_insert(4, 2, 0, 17, p16, p16, None) != 0 and b"nf must be in [1, 16]" in L.mw_last_error()
    assert L.mw_member_insert(4, 2, 0, 1, None, p16, None) != 0 and b"null pointer" in L.mw_last_error()
    assert L.mw_member_divergence(0, 2, 1, p16, one, one, one, None) != 0 and b"n must be >= 1" in L.mw_last_error()
    assert L.mw_member_divergence(4, 0, 1, p16, one, one, one, None) != 0 and b"nens must be in" in L.mw_last_error()
    assert L.mw_member_divergence(4, 2, 17, p16, one, one, one, None) != 0 and b"nf must be in [1, 16]" in L.mw_last_error()
    assert L.mw_member_divergence(4, 2, 1, p16, None, one, one, None) != 0 and b"null pointer" in L.mw_last_error()
    assert L.mw_surrogate_members_apply(None, members, 4, 16, 3, p16, None) != 0 and b"null pointer" in L.mw_last_error()
    assert L.mw_member_divergence_workspace_bytes(0, 2, 1) == 0 and L.mw_member_divergence_workspace_bytes(4, 2, 17) == 0
    # the partial sums: one row of 8 per block, field and member; blocks = cells / (256 / nens whole cells), at most 512
    assert L.mw_member_divergence_workspace_bytes(1, 2, 1) == 2 * 64
    assert L.mw_member_divergence_workspace_bytes(129, 2, 8) == 2 * 8 * 2 * 64
    assert L.mw_member_divergence_workspace_bytes(10 ** 9, 5, 8) == 512 * 8 * 5 * 64
    if torch.cuda.is_available():
        return
    assert L.mw_member_extract(4, 2, 0, 1, p16, p16, None) != 0 and b"no HIP device" in L.mw_last_error()
    assert L.mw_member_insert(4, 2, 0, 1, p16, p16, None) != 0 and b"no HIP device" in L.mw_last_error()
    assert L.mw_member_divergence(4, 2, 1, p16, one, one, one, None) != 0 and b"no HIP device" in L.mw_last_error()


# ---- the scorer's arithmetic --------------------------------------------------------------------------------------------------------
FIELDS = ("temp", "water_vapor", "cloud_liquid", "precip_liquid")


def raw_arrays(values):
    """member_divergence's arrays from host values (members, fields, cells): exactly rounded sums."""
    values = np.asarray(values, dtype=np.float64)
    nm, nf, n = values.shape
    stats, nonf = np.zeros((nm, nf, 7)), np.zeros((nm, nf), dtype=np.int64)
    for m in range(nm):
        for f in range(nf):
            x, d = values[m, f], values[m, f] - values[0, f]
            stats[m, f] = [math.fsum(d), math.fsum(np.abs(d)), math.fsum(d * d), np.max(np.abs(d)), math.fsum(x), np.min(x), np.max(x)]
            nonf[m, f] = np.count_nonzero(~np.isfinite(x))
    return stats, nonf


def test_report_arithmetic(mw):
    from miniweatherml_amd import modules
    rng = np.random.default_rng(0)
    v = rng.uniform(0.0, 1.0, (4, 4, 6))
    v[0, 0] = 300.0 + np.arange(6.0)                                     # (whole numbers: the differences below are exact)
    v[1, 0] = v[0, 0] + np.array([1.0, -1.0, 2.0, -2.0, 0.0, 0.0])
    v[3] = v[0]
    v[3, 0] = v[0, 0] + 2.0                                              # persistence: temp off by 2 everywhere, the water fields equal
    stats, nonf = raw_arrays(v)
    names = ["kessler", "a", "b", "persistence"]
    rep = modules.rollout_report(stats, nonf, 6, names, FIELDS, cell_volume=0.5, persistence=3)
    t = rep["a"]["fields"]["temp"]
    assert t["bias"] == 0.0 and t["mae"] == 1.0 and t["rmse"] == math.sqrt(10.0 / 6.0) and t["max_abs"] == 2.0
    assert t["rmse_over_persistence"] == math.sqrt(10.0 / 6.0) / 2.0 and "finite" not in t and t["nonfinite"] == 0
    assert t["mean"] == math.fsum(v[1, 0]) / 6.0 and t["min"] == v[1, 0].min() and t["max"] == v[1, 0].max()
    assert rep["persistence"]["fields"]["temp"]["rmse_over_persistence"] == 1.0
    # the persistence member's water equals Kessler's: rmse 0, no ratio for anybody
    assert rep["persistence"]["fields"]["water_vapor"]["rmse"] == 0.0
    assert all(rep[m]["fields"]["water_vapor"]["rmse_over_persistence"] is None for m in names)
    k = rep["kessler"]["fields"]["cloud_liquid"]
    assert (k["bias"], k["mae"], k["rmse"], k["max_abs"]) == (0.0, 0.0, 0.0, 0.0)
    for m, name in enumerate(names):
        assert rep[name]["total_water"] == (stats[m, 1, 4] + stats[m, 2, 4] + stats[m, 3, 4]) * 0.5 and rep[name]["finite"] is True
    # without a persistence member there is no ratio at all; without all three water fields no total
    rep = modules.rollout_report(stats[:3], nonf[:3], 6, names[:3], FIELDS)
    assert all(rep[m]["fields"][f]["rmse_over_persistence"] is None for m in names[:3] for f in FIELDS)
    rep = modules.rollout_report(stats[:, :2], nonf[:, :2], 6, names, FIELDS[:2], persistence=3)
    assert rep["a"]["total_water"] is None and rep["a"]["fields"]["temp"]["rmse_over_persistence"] is not None
    with pytest.raises(modules.MWError, match="stats must be"):
        modules.rollout_report(stats[:3], nonf, 6, names, FIELDS)


def test_scorer_keeps_the_first_non_finite_time_and_strict_json(mw):
    from miniweatherml_amd import modules
    rng = np.random.default_rng(1)
    v = rng.uniform(0.0, 1.0, (3, 4, 5))
    names = ["kessler", "sick", "persistence"]
    sc = modules.RolloutScorer(names, FIELDS)
    assert sc.persistence == 2 and modules.RolloutScorer(names[:2], FIELDS).persistence is None
    with pytest.raises(modules.MWError, match="nothing accumulated"):
        sc.report()
    sc.add(*raw_arrays(v), 5, 2.0, step=0, etime=0.5)
    assert sc.diverged_at == {"kessler": None, "sick": None, "persistence": None}
    for step in (2, 4):
        w = v.copy()
        w[1, 0, 3] = np.nan                                              # one NaN in the sick member's temp
        w[1, 2, 1] = np.inf                                              # and one inf in its cloud_liquid
        stats, nonf = raw_arrays(w)
        assert np.isnan(stats[1, 0, [0, 1, 2, 4]]).all() and nonf[1].tolist() == [1, 0, 1, 0]
        stats[1, 0, [3, 5, 6]] = np.nan                                  # (what the kernel's NaN-propagating extrema give; np.max does too)
        sc.add(stats, nonf, 5, 2.0, step=step, etime=0.5 * (step + 1))
    rep = sc.report()
    assert rep["diverged_at"] == {"kessler": None, "sick": {"step": 2, "etime": 1.5}, "persistence": None}
    assert [t["step"] for t in rep["times"]] == [0, 2, 4]
    sick = rep["times"][-1]["members"]["sick"]
    assert sick["finite"] is False and sick["total_water"] is None
    t = sick["fields"]["temp"]
    assert t["finite"] is False and t["nonfinite"] == 1 and all(t[k] is None for k in ("bias", "mae", "rmse", "max_abs", "mean", "min", "max"))
    c = sick["fields"]["cloud_liquid"]
    assert c["finite"] is False and c["max"] is None and c["min"] is not None
    assert "finite" not in sick["fields"]["water_vapor"] and rep["times"][-1]["members"]["persistence"]["finite"] is True
    assert rep["times"][0]["members"]["sick"]["finite"] is True
    text = json.dumps({"report": rep, "history": sc.history}, allow_nan=False)                # strict JSON: no bare NaN / Infinity token
    assert '"nan"' in text and '"inf"' in text
    back = json.loads(text)
    assert back["history"][0]["stats"] == raw_arrays(v)[0].tolist()
    table = sc.table()
    assert "sick" in table and "step 2" in table and "step 4" in table.splitlines()[0]
