"""The domain-split surrogate evaluation without a GPU: the `eval_domain:` key, the report's arithmetic on hand-made
exact sums, the numpy reference's own invariants, and the C entry points' argument refusals."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import eval_domain_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mw_surrogate_bank_set_domain", "mw_surrogate_eval_domain_group", "mw_surrogate_eval_domain")
ONE = 1 << 1074


def test_header_binding_table_and_exports_agree(mw):
    from miniweatherml_amd import capi
    header = open(os.path.join(ROOT, "include", "mw_cdna4.h")).read()
    L = C.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SYMBOLS and hasattr(L, name), name


def test_kernels_are_in_the_library_under_their_own_names(mw):
    import conftest
    from miniweatherml_amd import capi
    names = set()
    for m in re.finditer(rb"_ZN2mw(\d+)([0-9A-Za-z_]+)\.kd\x00", open(capi.LIB_PATH, "rb").read()):
        names.add(m.group(2)[:int(m.group(1))].decode())
    new = {"k_surrogate_eval_domain", "k_surrogate_eval_domain_stencil", "k_surrogate_eval_domain_strict", "k_surrogate_eval_domain_final"}
    assert new <= names and not (new & conftest._DISPATCHED)


def test_argument_refusals_come_before_the_device_check(mw):
    from miniweatherml_amd import capi
    L = capi.lib()
    fields = (C.c_void_p * 5)(*([0x1000] * 5))
    holed = (C.c_void_p * 5)(0x1000, 0x1000, 0, 0x1000, 0x1000)
    h, p = C.c_void_p(0x1000), C.c_void_p(0x1000)
    box = (C.c_double * 10)(*([0.0, 1.0] * 5))
    assert L.mw_surrogate_eval_domain(None, 4, 16, fields, fields, p, p, None) != 0 and b"null pointer" in L.mw_last_error()
    assert L.mw_surrogate_eval_domain(h, 4, 16, None, fields, p, p, None) != 0 and b"null pointer" in L.mw_last_error()
    assert L.mw_surrogate_eval_domain(h, 4, 16, fields, None, p, p, None) != 0 and b"null pointer" in L.mw_last_error()
    assert L.mw_surrogate_eval_domain(h, 4, 16, fields, fields, None, p, None) != 0 and b"null pointer" in L.mw_last_error()
    assert L.mw_surrogate_eval_domain(h, 4, 16, fields, fields, p, None, None) != 0 and b"null pointer" in L.mw_last_error()
    assert L.mw_surrogate_eval_domain(h, 0, 16, fields, fields, p, p, None) != 0 and b"nz and ncol" in L.mw_last_error()
    assert L.mw_surrogate_eval_domain(h, 4, 0, fields, fields, p, p, None) != 0 and b"nz and ncol" in L.mw_last_error()
    assert L.mw_surrogate_eval_domain(h, 4, 16, holed, fields, p, p, None) != 0 and b"null field" in L.mw_last_error()
    assert L.mw_surrogate_eval_domain(h, 4, 16, fields, holed, p, p, None) != 0 and b"null field" in L.mw_last_error()
    assert L.mw_surrogate_bank_set_domain(None, box) != 0 and b"null pointer" in L.mw_last_error()
    assert L.mw_surrogate_bank_set_domain(h, None) != 0 and b"null pointer" in L.mw_last_error()
    assert L.mw_surrogate_eval_domain_group(None) == 0 and b"null handle" in L.mw_last_error()
    import torch
    if not torch.cuda.is_available():
        assert L.mw_surrogate_eval_domain(h, 4, 16, fields, fields, p, p, None) != 0 and b"no HIP device" in L.mw_last_error()


def test_eval_domain_config():
    from miniweatherml_amd.surrogate_eval import eval_domain_config
    from miniweatherml_amd import driver
    names = ["parent", "child"]
    assert eval_domain_config(True, names) == {"margin": 0.0, "fields": list(ref.IN5), "box_of": None}
    got = eval_domain_config({"margin": 0.25, "fields": ["water_vapor", "temp"], "box_of": "parent"}, names)
    assert got == {"margin": 0.25, "fields": ["temp", "water_vapor"], "box_of": "parent"}
    with pytest.raises(ValueError, match="unknown key.*'boxof'"):
        eval_domain_config({"boxof": "parent"}, names)
    with pytest.raises(ValueError, match="box_of must name one of surrogate_models"):
        eval_domain_config({"box_of": "uncle"}, names)
    with pytest.raises(ValueError, match="box_of must name"):
        eval_domain_config({"box_of": 3}, names)
    with pytest.raises(ValueError, match="eval_domain.margin must be a finite number >= 0"):
        eval_domain_config({"margin": -0.1}, names)
    with pytest.raises(ValueError, match="eval_domain.margin"):
        eval_domain_config({"margin": True}, names)
    with pytest.raises(ValueError, match="eval_domain.fields must be a non-empty list"):
        eval_domain_config({"fields": ["rain"]}, names)
    with pytest.raises(ValueError, match="eval_domain.fields"):
        eval_domain_config({"fields": []}, names)
    with pytest.raises(ValueError, match="must be true or a mapping"):
        eval_domain_config(3, names)
    # the driver's reading of the key: absent or false is off
    assert driver.eval_domain_key({}, names) is None and driver.eval_domain_key({"eval_domain": False}, names) is None
    assert driver.eval_domain_key({"eval_domain": True}, names)["box_of"] is None


def test_load_config_keeps_the_key(tmp_path):
    from miniweatherml_amd import driver
    base = ("sim_time: 1.0\nnx_glob: 4\nny_glob: 4\nnz: 4\nxlen: 1.0\nylen: 1.0\nzlen: 1.0\ndt_phys: 0.0\nout_prefix: t\ninit_data: supercell\n"
            "out_freq: -1\n")
    p = tmp_path / "a.yaml"
    p.write_text(base + "eval_domain: {box_of: a, margin: 0.5}\n")
    assert driver.load_config(str(p))["eval_domain"] == {"box_of": "a", "margin": 0.5}
    p.write_text(base)
    assert "eval_domain" not in driver.load_config(str(p))


def hand_result(k=1):
    """A domain_scores dict of k models with all-zero sums and counts, to be filled by hand."""
    return {"sums": np.zeros((k, 2, 2, 2, 4, 3), dtype=object), "nonfinite": np.zeros((k, 2, 2, 2, 4, 3)), "max": np.zeros((k, 2, 2, 2, 4)),
            "counts": np.zeros((k, 2, 2), dtype=np.int64), "calls": 1}


def test_report_from_hand_made_sums():
    from miniweatherml_amd.surrogate_eval import domain_split_report
    r = hand_result()
    box = np.array([[250.0, 300.0], [0.1, 1.2], [0.0, 0.02], [0.0, np.inf], [-np.inf, np.inf]])
    # inside: 3 inactive and 1 active cell; outside: 0 inactive, 2 active.  field temp (0):
    r["counts"][0] = [[3, 1], [0, 2]]
    u = lambda x: int(Fraction(x) * ONE)                                   # noqa: E731   (x a dyadic rational: exact)
    # prediction [kind 0]: sums (sum d, sum |d|, sum d^2)
    r["sums"][0, 0, 0, 0, 0] = [u(-1.5), u(1.5), u(0.75)]                  # inside inactive
    r["sums"][0, 0, 0, 1, 0] = [u(2), u(2), u(4)]                          # inside active
    r["sums"][0, 0, 1, 1, 0] = [u(4), u(6), u(20)]                         # outside active
    r["max"][0, 0, 0, 0, 0], r["max"][0, 0, 0, 1, 0], r["max"][0, 0, 1, 1, 0] = 0.5, 2.0, 4.0
    # persistence [kind 1]: inside inactive exactly zero (rmse 0 -> no ratio), inside active sum d^2 = 16, outside active 5
    r["sums"][0, 1, 0, 1, 0] = [u(4), u(4), u(16)]
    r["sums"][0, 1, 1, 1, 0] = [u(1), u(3), u(5)]
    # field water_vapor (1): a NaN sum of d^2 outside active
    r["nonfinite"][0, 0, 1, 1, 1, 2] = np.nan
    r["max"][0, 0, 1, 1, 1] = np.nan
    rep = domain_split_report(["m"], [box], [r])["m"]
    assert rep["box"] == {"temp": [250.0, 300.0], "density_dry": [0.1, 1.2], "water_vapor": [0.0, 0.02], "cloud_liquid": [0.0, "inf"],
                          "precip_liquid": ["-inf", "inf"]}
    ins, out = rep["inside"], rep["outside"]
    assert [ins[c]["n"] for c in ("inactive", "active", "all")] == [3, 1, 4] and [out[c]["n"] for c in ("inactive", "active", "all")] == [0, 2, 2]
    t = ins["inactive"]["temp"]
    assert (t["bias"], t["mae"], t["rmse"], t["max_abs"]) == (-0.5, 0.5, 0.5, 0.5) and t["rmse_over_persistence"] is None      # persistence rmse 0
    t = ins["active"]["temp"]
    assert (t["bias"], t["mae"], t["rmse"], t["max_abs"], t["rmse_over_persistence"]) == (2.0, 2.0, 2.0, 2.0, 0.5)
    t = ins["all"]["temp"]                                                  # 4 cells, sum d^2 = 4.75; persistence 16
    assert t["bias"] == 0.125 and t["max_abs"] == 2.0 and t["rmse"] == np.sqrt(4.75 / 4) and t["rmse_over_persistence"] == np.sqrt(4.75 / 4) / 2.0
    t = out["active"]["temp"]
    assert (t["bias"], t["mae"], t["rmse"], t["max_abs"]) == (2.0, 3.0, np.sqrt(10.0), 4.0) and t["rmse_over_persistence"] == 2.0
    # an empty side-class: n = 0 and None everywhere
    assert out["inactive"]["temp"] == {"bias": None, "mae": None, "rmse": None, "max_abs": None, "rmse_over_persistence": None}
    # the non-finite sum: None and the flag, in its class and in `all`
    w = out["active"]["water_vapor"]
    assert w["rmse"] is None and w["max_abs"] is None and w["finite"] is False and w["bias"] == 0.0
    assert out["all"]["water_vapor"]["finite"] is False and "finite" not in ins["all"]["water_vapor"]
    # the share, an exact ratio of the integers
    share = rep["outside_share_of_squared_error"]
    assert share["active"]["temp"] == 20 / 24 and share["inactive"]["temp"] == 0.0 and share["all"]["temp"] == 20 / 24.75
    assert share["active"]["water_vapor"] is None and share["all"]["water_vapor"] is None
    assert share["inactive"]["water_vapor"] is None                         # 0 / 0
    # a ratio no fp64 division of rounded sums would give: (2^-1074) / (2^-1074 + 1)
    r2 = hand_result()
    r2["counts"][0] = [[1, 0], [1, 0]]
    r2["sums"][0, 0, 0, 0, 0, 2], r2["sums"][0, 0, 1, 0, 0, 2] = ONE, 1
    s = domain_split_report(["m"], [box], [r2])["m"]["outside_share_of_squared_error"]["inactive"]["temp"]
    assert s == 1 / (ONE + 1) and s > 0.0


def test_combine_is_exact_and_order_free():
    from miniweatherml_amd.surrogate_eval import DomainSplitEvaluator, domain_scores
    rng = np.random.default_rng(3)
    parts = []
    for _ in range(3):
        stats = rng.normal(size=(2, 2, 2, 2, 4, 4)) * 10.0 ** rng.integers(-12, 12, size=(2, 2, 2, 2, 4, 4))
        parts.append([domain_scores(stats, rng.integers(0, 100, size=(2, 2, 2)))])
    cmb = DomainSplitEvaluator.combine
    a, b = cmb(cmb(parts[0], parts[1]), parts[2]), cmb(parts[0], cmb(parts[1], parts[2]))
    assert np.array_equal(a[0]["sums"], b[0]["sums"]) and np.array_equal(a[0]["counts"], b[0]["counts"]) and a[0]["calls"] == 3
    assert a[0]["sums"].shape == (2, 2, 2, 2, 4, 3) and a[0]["max"].shape == (2, 2, 2, 2, 4)


@pytest.mark.parametrize("n_in", [5, 9])
def test_reference_invariants(n_in):
    """The sides partition the cells; an unbounded box puts everything inside; NaN, bounds, -0.0 and infinities follow the rule."""
    rng = np.random.default_rng(n_in)
    nz, ncol = 6, 11
    ins = [np.round(rng.uniform(0.0, 1.0, (nz, ncol)) * 2.0 ** 20) / 2.0 ** 20 for _ in range(5)]     # (dyadic: the differences below are exact)
    truth = [ins[i] + np.where(rng.random((nz, ncol)) < 0.5, 2.0 ** -10, 0.0) for i in ref.BEFORE]
    box = np.array([[0.1, 0.9]] * 5)
    stats, bound, counts = ref.model_rows(n_in, ins, truth, [t + 0.25 for t in truth], box)
    assert counts.sum() == nz * ncol and counts[0].sum() > 0 and counts[1].sum() > 0
    act = ref.active_mask(ins, truth)
    assert counts[:, 1].sum() == act.sum() and counts[:, 0].sum() == (~act).sum()
    assert np.all(stats[0, :, :, :, 3][counts > 0] == 0.25) and np.all(stats[0, :, :, :, 3][counts == 0] == 0.0)
    open_box = np.array([[-np.inf, np.inf]] * 5)
    assert not ref.outside_mask(n_in, ins, open_box).any()
    _, _, c2 = ref.model_rows(n_in, ins, truth, truth, open_box)
    assert c2[1].sum() == 0 and c2[0].sum() == nz * ncol
    # the rule, value by value, on field 3 of level 0 and of the top level
    box = np.array([[-np.inf, np.inf]] * 3 + [[0.0, 0.5]] + [[-np.inf, np.inf]])
    for k in (0, nz - 1):
        for x, want in ((0.0, False), (-0.0, False), (0.5, False), (np.nextafter(0.5, 1.0), True), (-5e-324, True), (np.nan, True),
                        (np.inf, True), (-np.inf, True)):
            f = [np.full((nz, ncol), 0.25) for _ in range(5)]
            f[3][k, 4] = x
            m = ref.outside_mask(n_in, f, box)
            expect = np.zeros((nz, ncol), bool)
            expect[k, 4] = want
            if n_in == 9 and k > 0:
                expect[k - 1, 4] = want                                   # through its level above
            assert np.array_equal(m, expect), (k, x)
    f = [np.full((nz, ncol), np.inf) for _ in range(5)]
    assert not ref.outside_mask(n_in, f, open_box).any()                   # +inf against an infinite bound is inside
