"""The training-domain guard without a GPU: the box of a model and of a committee against its numpy statement, the
`domain:` and `training_domain:` keys and what is refused, the report assembled from hand-made count arrays, and the new entry point in
the header, the binding table and the library with its argument refusals, which come before the device check."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import domain_ref
from test_surrogate_committee_cpu import BASE, model_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN5 = domain_ref.IN5


def model(scl_in, form="state"):
    from miniweatherml_amd import modules
    n_in = np.shape(scl_in)[0]
    return modules.SurrogateModel(np.zeros((n_in, 10), np.float32), np.zeros(10, np.float32), np.zeros((10, 4), np.float32), np.zeros(4, np.float32),
                                  np.asarray(scl_in, dtype=np.float64), np.array([[0.0, 1.0]] * 4), form)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


SINGLE = np.array([[200.0, 320.0], [0.1, 1.2], [0.0, 0.02], [0.0, 3.0e-3], [0.0, 7.0e-3]])
# the rows of the level above: temp narrower from below, cloud narrower from above, the other two wider on both sides
STENCIL = np.concatenate([SINGLE, [[210.0, 330.0], [-1.0, 0.03], [-1.0, 2.5e-3], [-1.0e-3, 8.0e-3]]])


# ---- domain_box ---------------------------------------------------------------------------------------------------------------------------
def test_box_of_a_single_cell_model():
    from miniweatherml_amd import modules
    box = modules.domain_box([model(SINGLE)])
    assert box.shape == (5, 2) and box.dtype == np.float64
    assert np.array_equal(bits(box), bits(SINGLE)) and np.array_equal(bits(box), bits(domain_ref.box_of([SINGLE])))
    assert np.array_equal(bits(modules.domain_box([tuple(model(SINGLE))[:6]])), bits(SINGLE))           # the six-tuple form too


def test_box_of_a_stencil_model_intersects_the_rows_of_the_level_above():
    from miniweatherml_amd import modules
    box = modules.domain_box([model(STENCIL)])
    want = SINGLE.copy()
    want[0, 0] = 210.0                     # temp: the level above starts higher
    want[3, 1] = 2.5e-3                    # cloud_liquid: the level above ends lower
    assert np.array_equal(bits(box), bits(want)) and np.array_equal(bits(box), bits(domain_ref.box_of([STENCIL])))
    assert np.array_equal(bits(box[1]), bits(SINGLE[1]))                                                 # density_dry has one row only


def test_box_of_a_committee_of_three_and_the_margin_bit_for_bit():
    from miniweatherml_amd import modules
    rng = np.random.default_rng(3)
    tables = [SINGLE + np.stack([rng.uniform(-0.1, 0.1, 5), rng.uniform(-0.1, 0.1, 5)], axis=1) * (SINGLE[:, 1] - SINGLE[:, 0])[:, None]
              for _ in range(3)]
    models = [model(t) for t in tables]
    box = modules.domain_box(models)
    lo, hi = np.max([t[:, 0] for t in tables], axis=0), np.min([t[:, 1] for t in tables], axis=0)
    assert np.array_equal(bits(box), bits(np.stack([lo, hi], axis=1)))
    for m in (0.05, 0.1, 1.0 / 3.0, 1.0e6):
        got = modules.domain_box(models, margin=m)
        w = hi - lo
        want = np.stack([lo - np.float64(m) * w, hi + np.float64(m) * w], axis=1)                        # the written formula, in fp64
        assert np.array_equal(bits(got), bits(want)), m
        assert np.array_equal(bits(got), bits(domain_ref.box_of(tables, m))), m
    nine = [model(np.concatenate([t, t[[0, 2, 3, 4]]])) for t in tables]
    assert np.array_equal(bits(modules.domain_box(nine, 0.05)), bits(modules.domain_box(models, 0.05)))


def test_a_fields_subset_leaves_the_others_unbounded():
    from miniweatherml_amd import modules
    box = modules.domain_box([model(STENCIL)], 0.1, fields=["water_vapor", "temp"])
    want = domain_ref.box_of([STENCIL], 0.1, ["temp", "water_vapor"])
    assert np.array_equal(bits(box), bits(want))
    for f in (1, 3, 4):
        assert box[f, 0] == -math.inf and box[f, 1] == math.inf
    assert np.isfinite(box[[0, 2]]).all()


def test_disjoint_ranges_are_refused_with_the_fields_name():
    from miniweatherml_amd import modules
    other = SINGLE.copy()
    other[3] = [4.0e-3, 5.0e-3]                                                                          # cloud_liquid beyond the first model's
    with pytest.raises(ValueError, match=r"cloud_liquid.*left, right"):
        modules.domain_box([model(SINGLE), model(other)], names=["left", "right"])
    with pytest.raises(ValueError, match="empty box for cloud_liquid"):
        domain_ref.box_of([SINGLE, other])
    assert np.isinf(modules.domain_box([model(SINGLE), model(other)], fields=["temp"])[3]).all()        # ... unless the field is left out
    inner = STENCIL.copy()
    inner[8] = [8.0e-3, 9.0e-3]                                                                          # a stencil model against itself
    with pytest.raises(ValueError, match="precip_liquid"):
        modules.domain_box([model(inner)])
    with pytest.raises(ValueError, match="all"):
        modules.domain_box([model(SINGLE), model(STENCIL)])


# ---- domain_config, guard_config --------------------------------------------------------------------------------------------------------
def test_domain_config():
    from miniweatherml_amd import modules
    assert modules.domain_config(True, "x") == {"margin": 0.0, "fields": list(IN5)}
    assert modules.domain_config({}, "x") == {"margin": 0.0, "fields": list(IN5)}
    got = modules.domain_config({"margin": 1, "fields": ["precip_liquid", "temp"]}, "x")
    assert got == {"margin": 1.0, "fields": ["temp", "precip_liquid"]} and isinstance(got["margin"], float)
    for bad, match in ((False, "true or a mapping"), (None, "true or a mapping"), (5, "true or a mapping"), ([1], "true or a mapping"),
                       ({"margins": 1}, r"unknown key\(s\) 'margins' in x"), ({"margin": -0.1}, "x.margin"), ({"margin": True}, "x.margin"),
                       ({"margin": "1"}, "x.margin"), ({"margin": math.nan}, "x.margin"), ({"fields": []}, "x.fields"),
                       ({"fields": "temp"}, "x.fields"), ({"fields": ["temp", "temp"]}, "x.fields"), ({"fields": ["uvel"]}, "x.fields"),
                       ({"fields": [1]}, "x.fields")):
        with pytest.raises(ValueError, match=match):
            modules.domain_config(bad, "x")


def test_guard_config_with_a_domain():
    from miniweatherml_amd import modules
    plain = {"temp": 2.0, "water_vapor": math.inf, "cloud_liquid": math.inf, "precip_liquid": math.inf, "max_rainsplit": 64}
    assert modules.guard_config({"temp": 2}) == plain                                                    # exactly today's dict: no new key
    got = modules.guard_config({"domain": True})
    assert got == dict(plain, temp=math.inf, domain={"margin": 0.0, "fields": list(IN5)})                # no threshold is needed beside it
    got = modules.guard_config({"temp": 2, "domain": {"margin": 0.5, "fields": ["temp"]}, "max_rainsplit": 8})
    assert got == dict(plain, max_rainsplit=8, domain={"margin": 0.5, "fields": ["temp"]})
    with pytest.raises(ValueError, match="no threshold"):
        modules.guard_config({})
    with pytest.raises(ValueError, match="no threshold"):
        modules.guard_config({"max_rainsplit": 8})
    with pytest.raises(ValueError, match=r"g\.domain must be true or a mapping"):
        modules.guard_config({"domain": False}, "g")
    with pytest.raises(ValueError, match=r"unknown key\(s\) 'box' in g\.domain"):
        modules.guard_config({"temp": 1, "domain": {"box": 1}}, "g")
    with pytest.raises(ValueError, match=r"unknown key\(s\) 'domains' in g"):
        modules.guard_config({"temp": 1, "domains": True}, "g")


# ---- the YAML keys ------------------------------------------------------------------------------------------------------------------------
def test_yaml_keys(mw, tmp_path):
    from miniweatherml_amd import driver
    lst, models = model_list(tmp_path, 2)
    p = tmp_path / "in.yaml"
    com = "surrogate_committees:\n  - {name: one, members: [model_1], guard: {domain: {margin: 0.25, fields: [temp, water_vapor]}}}\n" \
          "  - {name: two, members: [model_0, model_1], guard: {temp: 0.5, domain: true}}\n  - {name: plain, members: [model_0]}\n"
    p.write_text(BASE + lst + com)
    cfg = driver.load_config(str(p))
    got = driver.committee_config(cfg)
    assert got[0]["guard"]["domain"] == {"margin": 0.25, "fields": ["temp", "water_vapor"]} and got[0]["guard"]["temp"] == math.inf
    assert got[1]["guard"]["domain"] == {"margin": 0.0, "fields": list(IN5)} and got[1]["guard"]["temp"] == 0.5
    assert got[2] == {"name": "plain", "members": ["model_0"]}
    assert driver.rollout_config(cfg) == (models, 1, True, 7)                                            # Kessler + 2 + 3 committees + persistence
    assert driver.training_domain_config(cfg) is None and "training_domain" not in cfg
    for text, want in (("training_domain: true\n", {"margin": 0.0, "fields": list(IN5)}), ("training_domain: false\n", None),
                       ("training_domain: {margin: 0.1}\n", {"margin": 0.1, "fields": list(IN5)}),
                       ("training_domain: {fields: [precip_liquid]}\n", {"margin": 0.0, "fields": ["precip_liquid"]})):
        p.write_text(BASE + lst + com + text)
        cfg = driver.load_config(str(p))
        assert driver.training_domain_config(cfg) == want
        assert driver.rollout_config(cfg) == (models, 1, True, 7)                                        # the key adds no member
    for text, match in (("training_domain: 3\n", "training_domain must be true or a mapping"),
                        ("training_domain: {margin: -1}\n", "training_domain.margin"),
                        ("training_domain: {field: [temp]}\n", r"unknown key\(s\) 'field' in training_domain")):
        p.write_text(BASE + lst + text)
        with pytest.raises(ValueError, match=match):
            driver.training_domain_config(driver.load_config(str(p)))
    p.write_text(BASE + lst + "surrogate_committees:\n  - {name: c, members: [model_0], guard: {domain: {margin: x}}}\n")
    with pytest.raises(ValueError, match=r"the guard of committee 'c'\.domain\.margin"):
        driver.committee_config(driver.load_config(str(p)))
    with pytest.raises(ValueError, match=r"domain\.margin"):
        driver.rollout_config(driver.load_config(str(p)))


def test_evaluate_surrogates_refuses_a_guard_that_has_only_a_domain(mw, tmp_path):
    from miniweatherml_amd import driver
    lst, _ = model_list(tmp_path, 2)
    p = tmp_path / "in.yaml"
    p.write_text(BASE + lst + "surrogate_committees:\n  - {name: g, members: [model_0], guard: {domain: true}}\n")
    with pytest.raises(ValueError, match="does not apply a guard: committee 'g'"):
        driver.evaluation_committees(driver.load_config(str(p)))
    with pytest.raises(ValueError, match="does not apply a guard: committee 'g'"):
        driver.run("evaluate_surrogates", str(p), max_steps=1, quiet=True)


# ---- the report ---------------------------------------------------------------------------------------------------------------------------
def words(outside=0, **cells):
    """Sixteen count words from e.g. temp_above=3."""
    w = np.zeros(16, dtype=np.int64)
    for key, n in cells.items():
        f, c = key.rsplit("_", 1)
        w[3 * IN5.index(f) + ("below", "above", "nan").index(c)] = n
    w[15] = outside
    return w


def test_domain_report_from_hand_made_counts():
    from miniweatherml_amd import modules
    box = modules.domain_box([model(SINGLE)], fields=["temp", "precip_liquid"])
    cfg = modules.domain_config({"fields": ["precip_liquid", "temp"]}, "x")
    records = [(0, words()), (2, words(3, temp_above=4, precip_liquid_below=1)), (4, words(1, water_vapor_nan=2))]
    rep = modules.domain_report(cfg, box, 800, 100, records)
    assert list(rep) == ["margin", "fields", "box", "cells", "columns", "first_outside_step", "steps"]
    assert rep["margin"] == 0.0 and rep["fields"] == ["temp", "precip_liquid"] and rep["cells"] == 800 and rep["columns"] == 100
    assert rep["box"] == {"temp": [200.0, 320.0], "density_dry": ["-inf", "inf"], "water_vapor": ["-inf", "inf"], "cloud_liquid": ["-inf", "inf"],
                          "precip_liquid": [0.0, 7.0e-3]}
    assert rep["first_outside_step"] == 2 and [s["step"] for s in rep["steps"]] == [0, 2, 4]
    zero = {f: 0 for f in IN5}
    assert rep["steps"][0] == {"step": 0, "outside_columns": 0, "below": zero, "above": zero, "nan": zero}
    assert rep["steps"][1] == {"step": 2, "outside_columns": 3, "below": dict(zero, precip_liquid=1), "above": dict(zero, temp=4), "nan": zero}
    assert rep["steps"][2]["nan"] == dict(zero, water_vapor=2) and rep["steps"][2]["outside_columns"] == 1
    json.dumps(rep, allow_nan=False)
    assert modules.domain_report(cfg, box, 800, 100, records[:1])["first_outside_step"] is None
    assert modules.domain_report(cfg, box, 800, 100, [])["steps"] == []


def test_domain_reports_of_a_rollout_from_hand_made_counts():
    """Microphysics_Rollout.domain_reports on count arrays put where domain_record puts them: one block per network-stepped member, the
    committee's with the intersection of its models' boxes, None for kessler and persistence."""
    from miniweatherml_amd import modules
    narrow = SINGLE.copy()
    narrow[0] = [250.0, 300.0]
    micro = modules.Microphysics_Rollout.__new__(modules.Microphysics_Rollout)
    micro._models, micro._model_names, micro._committee_names = [model(SINGLE), model(narrow)], ["a", "b"], [("both", ["a", "b"])]
    micro.member_names = ["kessler", "a", "b", "both", "persistence"]
    micro._domain, micro._domain_counts, micro._domain_steps, micro._domain_cells = None, None, [], (96, 12)
    assert micro.domain_reports() == [None] * 5                                                          # without the attribute: nothing
    micro.training_domain = {"margin": 0.5}
    cfg, members, boxes = micro._domain_setup()
    assert members == [1, 2, 3] and boxes.shape == (3, 5, 2)
    micro._domain_steps = [(0, np.stack([words(), words(), words()])),
                           (3, np.stack([words(), words(2, temp_below=5), words(12, temp_nan=96)]))]
    rep = micro.domain_reports()
    assert rep[0] is None and rep[4] is None
    assert rep[1]["box"]["temp"] == [200.0 - 0.5 * 120.0, 320.0 + 0.5 * 120.0] and rep[1]["first_outside_step"] is None
    assert rep[2]["box"]["temp"] == rep[3]["box"]["temp"] == [225.0, 325.0]
    assert rep[2]["first_outside_step"] == 3 and rep[2]["steps"][1]["below"]["temp"] == 5 and rep[2]["steps"][1]["outside_columns"] == 2
    assert rep[3]["steps"][1]["nan"]["temp"] == 96 and rep[3]["cells"] == 96 and rep[3]["columns"] == 12 and rep[3]["margin"] == 0.5
    json.dumps(rep, allow_nan=False)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_exports_agree(mw):
    from miniweatherml_amd import capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mw_cdna4.h")).read(), flags=re.S)
    m = re.search(r"\bmw_member_domain\s*\(([^)]*)\)", header)
    assert m and len(m.group(1).split(",")) == 12
    assert len(capi.SYMBOLS["mw_member_domain"][1]) == 12 and hasattr(C.CDLL(capi.LIB_PATH), "mw_member_domain")
    assert capi.MW_DOMAIN_MAX_MEMBERS == 32 and capi.MW_DOMAIN_WORDS == 16


def refusal_cases():
    """(keyword changes of a valid call, a piece of the error text): every refusal the header lists."""
    def box(nm=2, at=None, value=0.0):
        b = np.tile(np.array([[-1.0, 1.0]]), (nm, 5, 1))
        if at is not None:
            b[at] = value
        return b
    return [(dict(in5=None), b"null pointer"), (dict(counts=None), b"null pointer"), (dict(box=None), b"null pointer"),
            (dict(members=None), b"null pointer"), (dict(nz=0), b"must be >= 1"), (dict(ncol=0), b"must be >= 1"), (dict(nens=0), b"nens must be"),
            (dict(nens=65), b"nens must be"), (dict(members=[]), b"nm must be"), (dict(nens=64, members=list(range(33)), box=box(33)), b"nm must be"),
            (dict(members=[1, 1]), b"listed twice"), (dict(members=[0, 3]), b"outside [0, 3)"), (dict(members=[-1, 0]), b"outside [0, 3)"),
            (dict(box=box(2, (1, 2, 0), 2.0)), b"not lo <= hi"), (dict(box=box(2, (0, 4, 1), math.nan)), b"not lo <= hi"),
            (dict(box=box(2, (0, 0, 0), math.nan)), b"not lo <= hi"), (dict(slots=[0, -1], flags=None), b"has a slot"),
            (dict(slots=[-1, 1], flag_counts=None), b"has a slot"), (dict(null_field=3), b"null field")]


def call_domain(L, fields, d_counts, d_flags, d_flag_counts, nz=4, ncol=16, nens=3, members=(2, 0), box=Ellipsis, slots=None, in5=Ellipsis,
                null_field=None, **over):
    """mw_member_domain with device addresses (or made-up ones) and the keyword changes of refusal_cases."""
    ptr = lambda v: None if v is None else C.c_void_p(v)                                                 # noqa: E731
    if box is Ellipsis:
        box = np.tile(np.array([[-1.0, 1.0]]), (max(1, len(members or ())), 5, 1))
    f5 = list(fields)
    if null_field is not None:
        f5[null_field] = None
    assert set(over) <= {"counts", "flags", "flag_counts"}, over
    counts, flags, flag_counts = over.get("counts", d_counts), over.get("flags", d_flags), over.get("flag_counts", d_flag_counts)
    return L.mw_member_domain(nz, ncol, nens, 0 if members is None else len(members),
                              None if members is None else (C.c_int * max(1, len(members)))(*members),
                              None if box is None else np.ascontiguousarray(box, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double)),
                              None if in5 is None else (C.c_void_p * 5)(*f5), ptr(counts), ptr(flags),
                              None if slots is None else (C.c_int * len(slots))(*slots), ptr(flag_counts), None)


def test_argument_refusals_come_before_the_device_check(mw):
    """Every pointer below is a made-up address: none of these calls may reach the device."""
    import torch
    from miniweatherml_amd import capi
    L = capi.lib()
    for kw, msg in refusal_cases():
        assert call_domain(L, [0x3000] * 5, 0x5000, 0x4000, 0x6000, **kw) != 0 and msg in L.mw_last_error(), kw
    if not torch.cuda.is_available():
        assert call_domain(L, [0x3000] * 5, 0x5000, 0x4000, 0x6000, slots=[0, 1]) != 0 and b"no HIP device" in L.mw_last_error()
