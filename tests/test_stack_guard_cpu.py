"""The guarded committee of dense stacks without a GPU: the `range_guard:` key of a `surrogate_committees` entry and
who refuses it, mw_stack_group_committee_guard_flag in the header, the binding table and the library, its argument refusals, which come
before the handle and the device are looked at, and CommitteeGuard(ranges=False) at a bank of fixed models.  (A group's handle needs a
device, so the refusal of a short workspace, which follows from the handle's plan, is in test_gpu_stack_guard.py.)"""
import ctypes as C
import math
import os
import re
import types

import pytest

from test_stack_members_cpu import config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, NARGS = "mw_stack_group_committee_guard_flag", 16


def entry(members=("deep", "wide"), **keys):
    return [dict({"name": "both", "members": list(members)}, **keys)]


def test_range_guard_is_returned_under_guard(tmp_path):
    from miniweatherml_amd import driver
    cfg, _ = config(tmp_path, stacks=("deep", "wide"), committees=entry(range_guard={"temp": 0.5, "max_rainsplit": 8}))
    assert driver.committee_config(cfg) == [{"name": "both", "members": ["deep", "wide"], "stacks": True, "guard": {
        "temp": 0.5, "water_vapor": math.inf, "cloud_liquid": math.inf, "precip_liquid": math.inf, "max_rainsplit": 8}}]
    assert "range_guard" in driver.COMMITTEE_KEYS


@pytest.mark.parametrize("case", ["fixed", "beside", "domain", "negative", "guard", "evaluate", "inference_ponni"])
def test_refusals_name_the_committee(tmp_path, case):
    from miniweatherml_amd import driver
    keys = {"beside": {"range_guard": {"temp": 1.0}, "guard": {"temp": 1.0}}, "domain": {"range_guard": {"temp": 1.0, "domain": True}},
            "negative": {"range_guard": {"temp": -1.0}}, "guard": {"guard": {"temp": 1.0}}}.get(case, {"range_guard": {"temp": 1.0}})
    cfg, _ = config(tmp_path, models=("a", "b"), stacks=("deep", "wide"), committees=entry(("a", "b") if case == "fixed" else ("deep", "wide"), **keys))
    match = {"fixed": "'both' has a range_guard and is a committee of surrogate_models", "beside": "'both' has a range_guard beside a guard",
             "domain": "range_guard of committee 'both' has a domain", "negative": "range_guard of committee 'both'.temp must be a number >= 0",
             "guard": "'both'.*has a guard.*range_guard", "evaluate": "does not apply a guard: committee 'both'",
             "inference_ponni": "inference_ponni.*'both'.*range_guard"}[case]
    with pytest.raises(ValueError, match=match):
        if case == "evaluate":
            driver.evaluation_committees(cfg)
        elif case == "inference_ponni":
            driver.InferencePonni().configure(cfg, 1)
        else:
            driver.committee_config(cfg)


def test_header_binding_table_and_exports_agree(mw):
    from miniweatherml_amd import capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mw_cdna4.h")).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)" % NAME, header)
    assert m and len(m.group(1).split(",")) == NARGS
    assert NAME in capi.SYMBOLS and len(capi.SYMBOLS[NAME][1]) == NARGS and hasattr(C.CDLL(capi.LIB_PATH), NAME)


def test_argument_refusals_come_before_the_handle_and_the_device(mw):
    """Every pointer is a made-up address and the handle is null: a call that passes every argument check ends at the null handle."""
    from miniweatherml_amd import capi
    L = capi.lib()
    ptrs = lambda vals: (C.c_void_p * len(vals))(*vals)      # noqa: E731
    thr = lambda *v: (C.c_double * 4)(*v)      # noqa: E731
    n = 4 * 16 * 3 * 8                                                           # bytes of a field
    f5, m4, r4 = ptrs([0x100000 + i * n for i in range(5)]), ptrs([0x200000 + i * n for i in range(4)]), ptrs([0x300000 + i * n for i in range(4)])

    def call(sel=(C.c_int * 2)(0, 1), member=1, nz=4, fields=f5, mean=m4, rng=r4, t=thr(1.0, math.inf, 0.0, 2.0), fl=C.c_void_p(0x4000), cnt=C.c_void_p(0x5000)):
        return L.mw_stack_group_committee_guard_flag(None, 2, sel, member, nz, 16, 3, fields, mean, rng, t, fl, cnt, None, 0, None)
    for kw, msg in ((dict(sel=None), b"null pointer"), (dict(fields=None), b"null pointer"), (dict(mean=None), b"null pointer"), (dict(t=None), b"null pointer"),
                    (dict(fl=None), b"null pointer"), (dict(cnt=None), b"null pointer"), (dict(mean=ptrs([0x200000, None, 0x210000, 0x220000])), b"null field"),
                    (dict(rng=ptrs([0x300000, 0x310000, None, 0x320000])), b"null field"), (dict(nz=0), b"must be >= 1"), (dict(member=3), b"outside [0, 3)"),
                    (dict(t=thr(1.0, -1.0, 1.0, 1.0)), b"threshold 1 is negative or NaN"), (dict(t=thr(1.0, 1.0, 1.0, math.nan)), b"threshold 3 is negative or NaN"),
                    (dict(mean=ptrs([0x100000] + [0x200000 + i * n for i in (1, 2, 3)])), b"in place is refused"),
                    (dict(mean=ptrs([0x200000 + i * n for i in range(3)] + [0x100000 + 4 * n + 8])), b"in place is refused"),
                    (dict(rng=ptrs([0x300000, 0x300000 + n - 8, 0x310000, 0x320000])), b"range fields must not overlap each other"),
                    (dict(rng=ptrs([0x200000 + n, 0x310000, 0x320000, 0x330000])), b"range field must not overlap a mean field"),
                    (dict(), b"null handle"), (dict(rng=None), b"null handle")):
        assert call(**kw) != 0 and msg in L.mw_last_error(), (kw, L.mw_last_error())


def test_a_scratch_without_ranges_is_refused_by_a_bank_of_fixed_models(mw):
    """CommitteeGuard(ranges=False) keeps no range4; SurrogateBank.committee_guard_flag, whose flags kernel reads the ranges, says so before
    it touches the device (the bank's own state is never reached: the method runs on a stand-in)."""
    import inspect
    from miniweatherml_amd import capi, mlp, modules
    assert inspect.signature(modules.CommitteeGuard.__init__).parameters["ranges"].default is True
    assert inspect.signature(mlp.MlpStackGroup.committee_guard_flag) == inspect.signature(modules.SurrogateBank.committee_guard_flag)
    assert inspect.signature(mlp.MlpStackGroup.committee_guard_apply) == inspect.signature(modules.SurrogateBank.committee_guard_apply)
    bank = types.SimpleNamespace(_member_layout=lambda who, nz, fields: (16, 3))
    guard = types.SimpleNamespace(range4=None, check_layout=lambda *a: None)
    with pytest.raises(capi.MWError, match="ranges=False"):
        modules.SurrogateBank.committee_guard_flag(bank, 4, [0, 1], 1, [None] * 5, [1.0] * 4, guard)
    with pytest.raises(capi.MWError, match="domain_box is not supported on a committee of stacks"):
        mlp.MlpStackGroup.committee_guard_flag(bank, 4, [0, 1], 1, [None] * 5, [1.0] * 4, guard, domain_box=[[0, 1]] * 5)
