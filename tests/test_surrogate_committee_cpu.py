"""The committee of surrogates without a GPU: the `surrogate_committees` key and what committee_config refuses, the member count a rollout
derives from it, the roles of the members, the argument checks of the two new entry points that come before the device check, the
combination rule (tests/committee_ref.py) on hand-computed cases, and the range / error correlation from its six sums."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mw_surrogate_committee_apply": 11, "mw_committee_score_workspace_bytes": 2, "mw_committee_score": 10}
BASE = "sim_time: 10\nnx_glob: 8\nny_glob: 8\nnz: 8\nxlen: 1\nylen: 1\nzlen: 1\ndt_phys: 0\nout_prefix: x\ninit_data: supercell\nout_freq: -1\n"


def model_list(tmp_path, k, stencil=0):
    """k single-cell models (named model_<i>) and `stencil` stencil models (stencil_<i>) as files: the YAML text of their list and the
    entries surrogate_config returns."""
    from miniweatherml_amd import modules, surrogate_train as st
    W1, b1, W2, b2, si, so = modules.load_surrogate_weights()
    w = st.initial_weights(0, k)
    _, models = st.write_outputs(str(tmp_path / "t"), w[0], si, so, {}, all_weights=w)
    if stencil:
        w9 = st.initial_weights(1, stencil, stencil=True)
        si9 = np.concatenate([si, si[[0, 2, 3, 4]]])
        _, m9 = st.write_outputs(str(tmp_path / "t9"), w9[0], si9, so, {}, all_weights=w9, names=["stencil_%d" % i for i in range(stencil)])
        models = models + m9
    return "surrogate_models:\n" + "".join("  - {%s}\n" % ", ".join('%s: "%s"' % kv for kv in m.items()) for m in models), models


def committees_yaml(entries):
    return "surrogate_committees:\n" + "".join("  - {name: %s, members: [%s]}\n" % (n, ", ".join(m)) for n, m in entries)


def test_valid_committees_are_returned_in_order(mw, tmp_path):
    from miniweatherml_amd import driver
    lst, models = model_list(tmp_path, 3, stencil=2)
    p = tmp_path / "in.yaml"
    p.write_text(BASE + lst + committees_yaml([("mean3", ["model_2", "model_0", "model_1"]), ("pair9", ["stencil_1", "stencil_0"]), ("one", ["model_1"])]))
    assert driver.committee_config(driver.load_config(str(p))) == [{"name": "mean3", "members": ["model_2", "model_0", "model_1"]},
                                                                   {"name": "pair9", "members": ["stencil_1", "stencil_0"]},
                                                                   {"name": "one", "members": ["model_1"]}]


def test_a_yaml_without_the_key_gives_todays_results(mw, tmp_path):
    from miniweatherml_amd import driver
    lst, models = model_list(tmp_path, 3)
    p = tmp_path / "in.yaml"
    p.write_text(BASE + lst + "harvest: {members: [model_1]}\n")
    cfg = driver.load_config(str(p))
    assert "surrogate_committees" not in cfg and driver.committee_config(cfg) == []
    assert driver.rollout_config(cfg) == (models, 1, True, 5)
    assert driver.surrogate_config(cfg) == (models, 1)
    assert driver.harvest_config(cfg)["members"] == ["model_1"]


@pytest.mark.parametrize("text,exc,match", [
    ("surrogate_committees: []\n", ValueError, "non-empty list"),
    ("surrogate_committees: 3\n", ValueError, "non-empty list"),
    ("surrogate_committees:\n  - [a]\n", KeyError, "'name' and 'members'"),
    ("surrogate_committees:\n  - {name: c}\n", KeyError, "'name' and 'members'"),
    ("surrogate_committees:\n  - {name: c, members: []}\n", ValueError, "non-empty list of model names"),
    ("surrogate_committees:\n  - {name: c, members: model_0}\n", ValueError, "non-empty list of model names"),
    ("surrogate_committees:\n  - {name: c, members: [model_0, nobody]}\n", ValueError, "'nobody', which is no surrogate model"),
    ("surrogate_committees:\n  - {name: c, members: [model_0, model_1, model_0]}\n", ValueError, "names a model twice"),
    ("surrogate_committees:\n  - {name: c, members: [model_0, stencil_0]}\n", ValueError, "one width"),
    ("surrogate_committees:\n  - {name: c, members: [model_0]}\n  - {name: c, members: [model_1]}\n", ValueError, "must be unique"),
    ("surrogate_committees:\n  - {name: model_1, members: [model_0]}\n", ValueError, "collides"),
    ("surrogate_committees:\n  - {name: kessler, members: [model_0]}\n", ValueError, "collides"),
    ("surrogate_committees:\n  - {name: persistence, members: [model_0]}\n", ValueError, "collides"),
    ("surrogate_committees:\n  - {name: c, members: [model_0], weights: [1]}\n", ValueError, "unknown key"),
])
def test_bad_committees_are_refused(mw, tmp_path, text, exc, match):
    from miniweatherml_amd import driver
    lst, _ = model_list(tmp_path, 2, stencil=1)
    p = tmp_path / "in.yaml"
    p.write_text(BASE + lst + text)
    with pytest.raises(exc, match=match):
        driver.committee_config(driver.load_config(str(p)))
    with pytest.raises(exc, match=match):                                      # the rollout's configuration runs the same checks
        driver.rollout_config(driver.load_config(str(p)))


def test_a_committee_holds_at_most_sixteen_models(mw, tmp_path):
    from miniweatherml_amd import capi, driver
    assert capi.MW_COMMITTEE_MAX_MODELS == 16
    lst, _ = model_list(tmp_path, 17)
    p = tmp_path / "in.yaml"
    p.write_text(BASE + lst + committees_yaml([("c", ["model_%d" % i for i in range(16)])]))
    assert len(driver.committee_config(driver.load_config(str(p)))[0]["members"]) == 16
    p.write_text(BASE + lst + committees_yaml([("c", ["model_%d" % i for i in range(17)])]))
    with pytest.raises(ValueError, match="at most 16"):
        driver.committee_config(driver.load_config(str(p)))
    p.write_text(BASE + committees_yaml([("c", ["model_0"])]))                   # committees need the list they name
    with pytest.raises(KeyError, match="surrogate_models"):
        driver.committee_config(driver.load_config(str(p)))


def test_rollout_members_count_the_committees(mw, tmp_path):
    from miniweatherml_amd import driver
    lst, models = model_list(tmp_path, 3)
    com = committees_yaml([("a", ["model_0", "model_1"]), ("b", ["model_2"])])
    p = tmp_path / "in.yaml"
    p.write_text(BASE + lst + com)
    assert driver.rollout_config(driver.load_config(str(p))) == (models, 1, True, 7)           # Kessler + 3 + 2 committees + persistence
    p.write_text(BASE + lst + com + "persistence_member: false\nnens: 6\n")
    assert driver.rollout_config(driver.load_config(str(p))) == (models, 1, False, 6)
    for bad in ("nens: 5\n", "nens: 8\n"):                                      # 5: right without the committees
        p.write_text(BASE + lst + com + bad)
        with pytest.raises(ValueError, match="2 surrogate_committees.*are 7 members \\(leave nens out\\)"):
            driver.rollout_config(driver.load_config(str(p)))


def test_the_member_limit_applies_to_the_total(mw, tmp_path):
    from miniweatherml_amd import driver
    lst, models = model_list(tmp_path, 26)
    p = tmp_path / "in.yaml"
    two = [("a", ["model_0", "model_1"]), ("b", ["model_2"])]
    p.write_text(BASE + lst + committees_yaml(two))                                # 1 + 26 + 2 + 1 = 30
    assert driver.rollout_config(driver.load_config(str(p)))[3] == 30
    p.write_text(BASE + lst + committees_yaml(two + [("c", ["model_3"])]))
    with pytest.raises(ValueError, match="3 surrogate_committees.*31 ensemble members, the dycore steps at most 30"):
        driver.rollout_config(driver.load_config(str(p)))


def test_harvest_refuses_a_committee(mw, tmp_path):
    from miniweatherml_amd import driver
    lst, _ = model_list(tmp_path, 2)
    p = tmp_path / "in.yaml"
    p.write_text(BASE + lst + committees_yaml([("both", ["model_0", "model_1"])]) + "harvest: {members: [model_0, both]}\n")
    with pytest.raises(ValueError, match="'both', which is a committee"):
        driver.harvest_config(driver.load_config(str(p)))
    p.write_text(BASE + lst + committees_yaml([("both", ["model_0", "model_1"])]) + "harvest: {members: [model_0]}\n")
    assert driver.harvest_config(driver.load_config(str(p)))["members"] == ["model_0"]


def test_member_names_with_committees():
    from miniweatherml_amd import capi, modules
    f = modules.rollout_member_names
    assert f(["a", "b"], True, ["c1", "c2"]) == ["kessler", "a", "b", "c1", "c2", "persistence"]
    assert f(["a", "b"], False, committees=["c1"]) == ["kessler", "a", "b", "c1"]
    assert f(["a", "b"]) == f(["a", "b"], True, ()) == ["kessler", "a", "b", "persistence"]
    for bad in (["c", "c"], ["a"], ["kessler"], ["persistence"]):
        with pytest.raises(capi.MWError, match="committee names must be unique and neither a model's name"):
            f(["a", "b"], True, bad)
    assert len(f(["m%d" % k for k in range(26)], True, ["x", "y"])) == 30
    with pytest.raises(capi.MWError, match="26 models, 3 committees and persistence beside Kessler are 31 ensemble members.*at most 30"):
        f(["m%d" % k for k in range(26)], True, ["x", "y", "z"])


def test_trainer_prints_a_committee_snippet():
    import yaml
    from miniweatherml_amd import surrogate_train as st
    doc = yaml.safe_load(st.committee_snippet(["seed0", "seed1", "seed2"]))
    assert doc == {"surrogate_committees": [{"name": "committee", "members": ["seed0", "seed1", "seed2"]}]}
    with pytest.raises(st.SurrogateTrainError, match="at most 16"):
        st.committee_snippet(["seed%d" % k for k in range(17)])


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
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
    assert int(re.search(r"#define MW_COMMITTEE_MAX_MODELS (\d+)", header).group(1)) == capi.MW_COMMITTEE_MAX_MODELS == 16


def _ptrs(vals):
    return (C.c_void_p * len(vals))(*vals)


def test_committee_apply_argument_errors_come_before_the_device_check(mw):
    """Without a bank (a bank needs a device) the checks that do not read it: null pointers, the committee's size, the shape, the member.
    The handle is a dummy address that these checks never follow."""
    from miniweatherml_amd import capi
    L = capi.lib()
    h = C.c_void_p(C.addressof(C.create_string_buffer(256)))
    sel, in5, out4 = (C.c_int * 17)(*range(17)), _ptrs([8] * 5), _ptrs([16] * 4)

    def err(*a):
        assert L.mw_surrogate_committee_apply(*a) != 0
        return L.mw_last_error().decode()
    assert "null pointer" in err(None, 2, sel, 0, 4, 16, 1, in5, out4, None, None)
    assert "null pointer" in err(h, 2, None, 0, 4, 16, 1, in5, out4, None, None)
    assert "null pointer" in err(h, 2, sel, 0, 4, 16, 1, None, out4, None, None)
    assert "null pointer" in err(h, 2, sel, 0, 4, 16, 1, in5, None, None, None)
    assert "1 to 16 models, got 0" in err(h, 0, sel, 0, 4, 16, 1, in5, out4, None, None)
    assert "1 to 16 models, got 17" in err(h, 17, sel, 0, 4, 16, 1, in5, out4, None, None)
    for nz, ncol, nens in ((0, 16, 1), (4, 0, 1), (4, 16, 0)):
        assert "must be >= 1" in err(h, 2, sel, 0, nz, ncol, nens, in5, out4, None, None)
    assert "member 3 is outside [0, 3)" in err(h, 2, sel, 3, 4, 16, 3, in5, out4, None, None)
    assert "member -1 is outside [0, 3)" in err(h, 2, sel, -1, 4, 16, 3, in5, out4, None, None)


def test_committee_score_argument_errors_come_before_the_device_check(mw):
    from miniweatherml_amd import capi
    L = capi.lib()
    f5, f4, one = _ptrs([8] * 5), _ptrs([8] * 4), C.c_void_p(8)
    assert L.mw_committee_score_workspace_bytes(0, 5) == 0 and L.mw_committee_score_workspace_bytes(4, 0) == 0
    assert L.mw_committee_score_workspace_bytes(1, 1) == 8 * (56 + 9)
    assert L.mw_committee_score_workspace_bytes(100, 400 * 400) == 1024 * 8 * (56 + 9)          # grid-stride beyond 1024 blocks
    good = [4, 16, f5, f4, f4, f4, one, one, one, None]

    def err(a):
        assert L.mw_committee_score(*a) != 0
        return L.mw_last_error().decode()
    for i in range(2, 9):
        assert "null pointer" in err(good[:i] + [None] + good[i + 1:]), i
    assert "must be >= 1" in err([0] + good[1:]) and "must be >= 1" in err([4, 0] + good[2:])
    for i in (2, 3, 4, 5):
        bad = list(good)
        bad[i] = _ptrs([8] * (len(good[i]) - 1) + [None])
        assert "null field" in err(bad), i
    if L.mw_device_count() < 1:
        assert "no HIP device" in err(good)


# ---- the combination rule ---------------------------------------------------------------------------------------------------------------
def test_the_order_of_three_addends_changes_the_last_bit():
    """1 + 2^-53 rounds back to 1 (a tie, to even), twice; 2^-53 + 2^-53 = 2^-52 survives the addition to 1.  Worked by hand:
    (1 + e) + e = 1, mean = fl(1 / 3) = 0x1.5555555555555p-2; (e + e) + 1 = 1 + 2^-52, mean = fl((1 + 2^-52) / 3): the exact quotient
    is 1/3 + 2^-52 / 3 = 0x1.5555555555556AAA...p-2 -> 0x1.5555555555557p-2 (its tail .AAA.. is above the half).  The range does not
    depend on the order: 1 - 2^-53 = 0x1.fffffffffffffp-1, exact."""
    from fractions import Fraction
    import committee_ref as R
    e = 2.0 ** -53
    m1, r1 = R.combine([np.array([1.0]), np.array([e]), np.array([e])])
    m2, r2 = R.combine([np.array([e]), np.array([e]), np.array([1.0])])
    assert float(m1[0]).hex() == "0x1.5555555555555p-2" and float(m2[0]).hex() == "0x1.5555555555557p-2"
    assert m1[0] == float(Fraction(1, 3)) and m2[0] == float((Fraction(1) + Fraction(1, 2 ** 52)) / 3)       # (float(Fraction) rounds correctly)
    assert float(r1[0]).hex() == float(r2[0]).hex() == "0x1.fffffffffffffp-1"


def test_a_committee_of_one_and_a_nan_member():
    import committee_ref as R
    y = np.array([1.0 / 3.0, -0.0, 5e-324, 1e308, np.inf])
    m, r = R.combine([y])
    assert np.array_equal(m.view(np.int64), y.view(np.int64)) and np.array_equal(r[:4], np.zeros(4)) and np.isnan(r[4])
    a, b, c = np.array([1.0, 2.0, 3.0]), np.array([4.0, np.nan, 1.0]), np.array([0.5, 7.0, 2.0])
    for ys in ([a, b, c], [b, a, c], [a, c, b]):                                # wherever the NaN member stands
        m, r = R.combine(ys)
        assert np.isnan(m[1]) and np.isnan(r[1])
        assert m[0] == sum(float(y[0]) for y in ys) / 3.0 and (r[0], r[2]) == (3.5, 2.0)
    assert R.same_bits(np.array([np.nan, 1.0]), np.array([-np.nan, 1.0])) and not R.same_bits(np.array([0.0]), np.array([-0.0]))
    assert not R.same_bits(np.array([np.nan, 1.0]), np.array([1.0, np.nan]))


def test_range_error_correlation_from_the_six_sums():
    from miniweatherml_amd import modules
    rng = np.random.default_rng(3)
    r = rng.uniform(0.0, 2.0, 500)
    a = np.abs(0.7 * r + rng.normal(0.0, 0.3, 500))
    got = modules.range_error_correlation(500, r.sum(), (r * r).sum(), a.sum(), (a * a).sum(), (r * a).sum())
    assert abs(got - np.corrcoef(r, a)[0, 1]) < 1e-12
    f = modules.range_error_correlation
    assert f(0, 0.0, 0.0, 0.0, 0.0, 0.0) is None
    assert f(4, 8.0, 16.0, 3.0, 5.0, 6.0) is None                              # a constant range (2, 2, 2, 2): no variance
    assert f(4, 6.0, 14.0, 0.0, 0.0, 0.0) is None                              # a perfect prediction
    assert f(4, np.nan, 14.0, 3.0, 5.0, 6.0) is None and f(4, 6.0, np.inf, 3.0, 5.0, 6.0) is None
