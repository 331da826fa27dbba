"""The guarded committee without a GPU: the `guard:` mapping of a `surrogate_committees` entry and what committee_config refuses, the member
count of a rollout with a guarded committee, the three new entry points in the header, the binding table and the library, and their
argument refusals, which come before the device check."""
import ctypes as C
import math
import os
import re

import pytest

from test_surrogate_committee_cpu import BASE, model_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mw_committee_guard_flags": 10, "mw_kessler_columns_teacher_workspace_bytes": 3, "mw_kessler_columns_teacher": 12, "mw_members_copy": 8}
FIELDS = ("temp", "water_vapor", "cloud_liquid", "precip_liquid")


def committee(guard=None, name="c", members="[model_0, model_1]"):
    return "  - {name: %s, members: %s%s}\n" % (name, members, "" if guard is None else ", guard: %s" % guard)


# ---- the YAML key -------------------------------------------------------------------------------------------------------------------------
def test_a_guard_is_accepted_and_completed(mw, tmp_path):
    from miniweatherml_amd import driver
    lst, models = model_list(tmp_path, 3)
    p = tmp_path / "in.yaml"
    p.write_text(BASE + lst + "surrogate_committees:\n" + committee() + committee("{precip_liquid: 1.0e-5, temp: 0.5}", "g") +
                 committee("{water_vapor: 0, cloud_liquid: .inf, max_rainsplit: 8}", "h"))
    got = driver.committee_config(driver.load_config(str(p)))
    assert got[0] == {"name": "c", "members": ["model_0", "model_1"]}           # an unguarded entry is what it was
    assert got[1] == {"name": "g", "members": ["model_0", "model_1"],           # the same models under a second name, guarded
                      "guard": {"temp": 0.5, "water_vapor": math.inf, "cloud_liquid": math.inf, "precip_liquid": 1.0e-5, "max_rainsplit": 64}}
    assert got[2]["guard"] == {"temp": math.inf, "water_vapor": 0.0, "cloud_liquid": math.inf, "precip_liquid": math.inf, "max_rainsplit": 8}


@pytest.mark.parametrize("guard,match", [
    ("{rain: 1}", r"unknown key\(s\) 'rain' in the guard of committee 'c'"),
    ("{temp: 1, threshold: 2}", r"unknown key\(s\) 'threshold' in the guard of committee 'c'"),
    ("{temp: -1}", "temp must be a number >= 0"),
    ("{precip_liquid: -0.5, temp: 1}", "precip_liquid must be a number >= 0"),
    ("{temp: big}", "temp must be a number >= 0"),
    ("{temp: true}", "temp must be a number >= 0"),
    ("{temp: .nan}", "temp must be a number >= 0"),
    ("{temp: [1]}", "temp must be a number >= 0"),
    ("{}", "no threshold"),
    ("{max_rainsplit: 8}", "no threshold"),
    ("{temp: 1, max_rainsplit: 0}", "max_rainsplit"),
    ("{temp: 1, max_rainsplit: 1025}", "max_rainsplit"),
    ("{temp: 1, max_rainsplit: 2.5}", "max_rainsplit"),
    ("5", "must be a mapping"),
    ("[1, 2]", "must be a mapping"),
])
def test_bad_guards_are_refused(mw, tmp_path, guard, match):
    from miniweatherml_amd import driver
    lst, _ = model_list(tmp_path, 2)
    p = tmp_path / "in.yaml"
    p.write_text(BASE + lst + "surrogate_committees:\n" + committee(guard))
    with pytest.raises(ValueError, match=match):
        driver.committee_config(driver.load_config(str(p)))
    with pytest.raises(ValueError, match=match):
        driver.rollout_config(driver.load_config(str(p)))


def test_a_guarded_committee_is_one_member_and_is_not_harvested(mw, tmp_path):
    from miniweatherml_amd import driver
    lst, models = model_list(tmp_path, 3)
    p = tmp_path / "in.yaml"
    text = BASE + lst + "surrogate_committees:\n" + committee() + committee("{temp: 1}", "g")
    p.write_text(text)
    assert driver.rollout_config(driver.load_config(str(p))) == (models, 1, True, 7)        # Kessler + 3 + 2 committees + persistence
    p.write_text(text + "harvest: {members: [g]}\n")
    with pytest.raises(ValueError, match="which is a committee"):
        driver.harvest_config(driver.load_config(str(p)))


def test_evaluate_surrogates_refuses_a_guard(mw, tmp_path):
    """evaluate_surrogates scores the mean: a guarded entry is refused before anything runs, an unguarded one is what it was."""
    from miniweatherml_amd import driver
    lst, _ = model_list(tmp_path, 2)
    p = tmp_path / "in.yaml"
    p.write_text(BASE + lst + "surrogate_committees:\n" + committee())
    assert driver.evaluation_committees(driver.load_config(str(p))) == [{"name": "c", "members": ["model_0", "model_1"]}]
    p.write_text(BASE + lst + "surrogate_committees:\n" + committee() + committee("{temp: 0.5}", "g"))
    with pytest.raises(ValueError, match="does not apply a guard: committee 'g'"):
        driver.evaluation_committees(driver.load_config(str(p)))
    with pytest.raises(ValueError, match="does not apply a guard: committee 'g'"):
        driver.run("evaluate_surrogates", str(p), max_steps=1, quiet=True)


def test_guard_config_alone():
    from miniweatherml_amd import modules
    assert modules.guard_config({"temp": 2}) == {"temp": 2.0, "water_vapor": math.inf, "cloud_liquid": math.inf, "precip_liquid": math.inf,
                                                 "max_rainsplit": 64}
    with pytest.raises(ValueError, match="no threshold"):
        modules.guard_config({})
    assert callable(modules.CommitteeGuard) and hasattr(modules.SurrogateBank, "committee_guard_apply")


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


def _ptrs(vals):
    return (C.c_void_p * len(vals))(*vals)


def test_argument_refusals_come_before_the_device_check(mw):
    """Every pointer below is a made-up address: none of these calls may reach the device."""
    import torch
    from miniweatherml_amd import capi
    L = capi.lib()
    m4, r4, f5 = _ptrs([0x1000] * 4), _ptrs([0x2000] * 4), _ptrs([0x3000] * 5)
    flags, counts, ws = C.c_void_p(0x4000), C.c_void_p(0x5000), C.c_void_p(0x6000)

    def thr(*v):
        return (C.c_double * 4)(*v)

    def gflags(nz=4, ncol=16, nens=3, member=1, mean=m4, rng=r4, t=thr(1.0, math.inf, 0.0, 2.0), fl=flags, cnt=counts):
        return L.mw_committee_guard_flags(nz, ncol, nens, member, mean, rng, t, fl, cnt, None)
    for kw, msg in ((dict(nz=0), b"must be >= 1"), (dict(ncol=0), b"must be >= 1"), (dict(member=3), b"outside [0, 3)"), (dict(member=-1), b"outside [0, 3)"),
                    (dict(t=thr(1.0, -1.0, 1.0, 1.0)), b"negative or NaN"), (dict(t=thr(1.0, 1.0, 1.0, math.nan)), b"negative or NaN"),
                    (dict(t=thr(-math.inf, 1.0, 1.0, 1.0)), b"negative or NaN"), (dict(mean=None), b"null pointer"), (dict(rng=None), b"null pointer"),
                    (dict(t=None), b"null pointer"), (dict(fl=None), b"null pointer"), (dict(cnt=None), b"null pointer"),
                    (dict(rng=_ptrs([0x2000, None, 0x2000, 0x2000])), b"null field")):
        assert gflags(**kw) != 0 and msg in L.mw_last_error(), kw

    assert L.mw_kessler_columns_teacher_workspace_bytes(10, 100, 3) == L.mw_kessler_members_teacher_workspace_bytes(10, 100, 3) > 0
    assert L.mw_kessler_columns_teacher_workspace_bytes(1, 100, 3) == 0 and L.mw_kessler_columns_teacher_workspace_bytes(10, 100, 65) == 0

    def teacher(nz=4, ncol=16, nens=3, fl=flags, dt=1.0, cap=64, fields=f5, outs=m4, work=ws):
        return L.mw_kessler_columns_teacher(nz, ncol, nens, fl, 500.0, dt, cap, fields, outs, None, work, None)
    for kw, msg in ((dict(nz=1), b"nz >= 2"), (dict(ncol=0), b"ncol >= 1"), (dict(nens=65), b"nens must be"), (dict(nens=0), b"nens must be"),
                    (dict(dt=0.0), b"nonpositive dt"), (dict(dt=math.nan), b"nonpositive dt"), (dict(cap=0), b"max_rainsplit"),
                    (dict(cap=1025), b"max_rainsplit"), (dict(fl=None), b"null pointer"), (dict(fields=None), b"null pointer"),
                    (dict(outs=None), b"null pointer"), (dict(work=None), b"null pointer"),
                    (dict(fields=_ptrs([0x3000, 0x3000, None, 0x3000, 0x3000])), b"null field")):
        assert teacher(**kw) != 0 and msg in L.mw_last_error(), kw

    def copy(n=64, nens=3, members=(1,), nf=4, src=m4, dst=r4):
        return L.mw_members_copy(n, nens, len(members), (C.c_int * max(1, len(members)))(*members), nf, src, dst, None)
    for kw, msg in ((dict(n=0), b"n must be"), (dict(nens=0), b"nens must be"), (dict(nens=65), b"nens must be"), (dict(members=()), b"nm must be"),
                    (dict(members=(0, 1, 2, 0)), b"nm must be"), (dict(members=(3,)), b"outside [0, 3)"), (dict(members=(1, 1)), b"listed twice"),
                    (dict(nf=0), b"nf must be"), (dict(src=None), b"null pointer"), (dict(dst=None), b"null pointer"),
                    (dict(dst=_ptrs([0x2000, 0x2000, None, 0x2000])), b"null field")):
        assert copy(**kw) != 0 and msg in L.mw_last_error(), kw
    assert L.mw_members_copy(64, 3, 1, None, 4, m4, r4, None) != 0 and b"null pointer" in L.mw_last_error()
    if not torch.cuda.is_available():
        assert gflags() != 0 and b"no HIP device" in L.mw_last_error()
        assert teacher() != 0 and b"no HIP device" in L.mw_last_error()
        assert copy() != 0 and b"no HIP device" in L.mw_last_error()
