"""Harvest outside the training box and the domain table that follows --init, without a GPU: the `harvest.outside`
key, harvest_thresholds against its restatement, training_domain.txt's union rule, its writer and reader, domain_box with tables, the
`nn_training_domain` key, the report blocks from hand-made counts, and the new entry point's refusals, which come before the device
check and leave mask and counts alone."""
import ctypes as C
import itertools
import json
import math
import os
import re

import numpy as np
import pytest

import harvest_domain_ref as ref
from test_domain_guard_cpu import SINGLE, STENCIL, bits, model
from test_surrogate_harvest_cpu import BASE, model_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN5 = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")


# ---- harvest.outside ------------------------------------------------------------------------------------------------------------------------
def test_harvest_outside_config(mw, tmp_path):
    from miniweatherml_amd import driver
    lst, models = model_list(tmp_path, 2)
    names = [m["name"] for m in models]
    p = tmp_path / "in.yaml"
    parent = {"interval": 4, "samples_per_step": 50, "ratio_active": 0.5, "seed": None, "max_rainsplit": 64, "members": names}
    p.write_text(BASE + lst + "eval_interval: 4\nharvest: {}\n")
    got = driver.harvest_config(driver.load_config(str(p)))
    assert got == parent and "outside" not in got                             # without the key: exactly the mapping it always was
    p.write_text(BASE + lst + "eval_interval: 4\nharvest: {outside: true}\n")
    assert driver.harvest_config(driver.load_config(str(p))) == dict(parent, outside={"share": 0.5, "margin": 0.0, "fields": list(IN5)})
    p.write_text(BASE + lst + "eval_interval: 4\nharvest: {outside: {share: 1, margin: 0.25, fields: [water_vapor, temp]}}\n")
    got = driver.harvest_config(driver.load_config(str(p)))["outside"]
    assert got == {"share": 1.0, "margin": 0.25, "fields": ["temp", "water_vapor"]} and isinstance(got["share"], float)
    for bad, msg in (("{share: 0}", r"share must be a number in \(0, 1\]"), ("{share: 1.5}", "share"), ("{share: true}", "share"),
                     ("{share: half}", "share"), ("{shares: 0.5}", r"unknown key\(s\) 'shares' in harvest.outside"),
                     ("{margin: -1}", r"harvest\.outside\.margin"), ("{margin: true}", r"harvest\.outside\.margin"),
                     ("{fields: [pressure]}", r"harvest\.outside\.fields"), ("{fields: []}", r"harvest\.outside\.fields"),
                     ("5", "true or a mapping"), ("[1]", "true or a mapping")):
        p.write_text(BASE + lst + "harvest: {outside: %s}\n" % bad)
        with pytest.raises(ValueError, match=msg):
            driver.harvest_config(driver.load_config(str(p)))


# ---- harvest_thresholds ---------------------------------------------------------------------------------------------------------------------
def test_harvest_thresholds_equal_their_restatement():
    from miniweatherml_amd import modules
    grid = itertools.product((50, 100, 333.5), (0.25, 0.5, 0.9), (0.4, 0.05), (1, 97, 73728, 16000000), (0.1, 0.5, 1.0 / 3.0, 1.0),
                             (0, 1, 49, 50, 51, 10 ** 7))
    for args in grid:
        got = modules.harvest_thresholds(*args)
        assert got == ref.harvest_thresholds(*args), args                      # the same expressions in the same order: the same doubles
        assert all(isinstance(x, float) and 0.0 <= x <= 1.0 for x in got), args
    ncell = 73728
    assert modules.harvest_thresholds(100, 0.5, 0.4, ncell, 0.5, 0)[0] == 0.0  # nothing outside: nothing is asked of the class
    assert modules.harvest_thresholds(100, 0.5, 0.4, ncell, 0.5, 49)[0] == 1.0 and modules.harvest_thresholds(100, 0.5, 0.4, ncell, 0.5, 50)[0] == 1.0
    assert modules.harvest_thresholds(100, 0.5, 0.4, ncell, 0.5, 200)[0] == 0.25
    assert modules.harvest_thresholds(100, 0.5, 0.4, 10, 0.5, 5) == (1.0, 1.0, 1.0)                      # ten cells: every rate clamps
    assert modules.harvest_thresholds(100, 0.5, 0.4, ncell, 1.0, 400) == (0.25, 0.0, 0.0)                # share 1: the inside classes get none
    assert modules.harvest_thresholds(100, 0.5, 0.4, ncell, 1, 400) == (0.25, 0.0, 0.0)
    # share 0.5 of 100 leaves exactly the plain harvester's 50
    plain = (min(1.0, 0.5 * 50.0 / (0.4 * ncell)), min(1.0, (1 - 0.5) * 50.0 / ((1 - 0.4) * ncell)))
    assert modules.harvest_thresholds(100.0, 0.5, 0.4, ncell, 0.5, 0)[1:] == plain


# ---- training_domain.txt --------------------------------------------------------------------------------------------------------------------
def awkward_rows(rng, n_in):
    """Rows of fp32-exact doubles (as data_scaling's), with a constant row and a negative one."""
    t = np.sort(rng.normal(size=(n_in, 2)).astype(np.float32).astype(np.float64), axis=1)
    t[1] = [0.5, 0.5]
    t[2] = [-3.0e-5, -1.0e-6]
    return t


@pytest.mark.parametrize("n_in", [5, 9])
def test_union_is_the_elementwise_min_and_max(n_in):
    from miniweatherml_amd import surrogate_train as st
    rng = np.random.default_rng(n_in)
    x = rng.normal(size=(40, n_in)).astype(np.float32)
    init_rows = awkward_rows(rng, n_in)
    init_rows[0] = [-100.0, 100.0]                                             # one row that the old table decides on both sides
    data_rows, _ = st.data_scaling(x, rng.normal(size=(40, 4)).astype(np.float32), allow_constant=True)
    got = st.training_domain_union(data_rows, init_rows)
    want = np.stack([np.minimum(x.min(axis=0).astype(np.float64), init_rows[:, 0]), np.maximum(x.max(axis=0).astype(np.float64), init_rows[:, 1])], axis=1)
    assert got.shape == (n_in, 2) and got.dtype == np.float64
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got), bits(ref.domain_union(x, init_rows)))
    assert (got[:, 0] <= init_rows[:, 0]).all() and (got[:, 1] >= init_rows[:, 1]).all()                # never narrower than either source
    assert (got[:, 0] < init_rows[:, 0]).any() and (got[:, 0] == init_rows[:, 0]).any()                 # and both sources show
    with pytest.raises(st.SurrogateTrainError, match="training domain"):
        st.training_domain_union(data_rows, init_rows[:-1])


@pytest.mark.parametrize("n_in", [5, 9])
def test_table_round_trips_and_the_directory_s_own_table_comes_first(mw, tmp_path, n_in):
    from miniweatherml_amd import modules, surrogate_train as st
    rng = np.random.default_rng(10 + n_in)
    rows = awkward_rows(rng, n_in)
    rows[0] = [1.0 / 3.0, 2.0e300]                                             # not fp32-exact: the text still reads back to the same double
    rows[3] = [-math.inf, math.inf]
    d = tmp_path / "m"
    path = st.write_training_domain(str(d), rows)
    assert path == str(d / "training_domain.txt")
    back = modules.load_training_domain(path, n_in)
    assert back.shape == (n_in, 2) and back.dtype == np.float64 and np.array_equal(bits(back), bits(rows))
    # init_domain: the scaling rows while the directory has no table of its own, the table once it has
    scl = awkward_rows(rng, n_in)
    e = tmp_path / "e"
    st.write_outputs(str(e), np.zeros(144 if n_in == 9 else 104, np.float32), scl, np.array([[0.0, 1.0]] * 4), {})
    assert np.array_equal(bits(st.init_domain(str(e), n_in)), bits(scl))
    st.write_training_domain(str(e), rows)
    assert np.array_equal(bits(st.init_domain(str(e), n_in)), bits(rows))
    assert np.array_equal(bits(np.loadtxt(str(e / "input_scaling.txt"))), bits(scl))                    # (which the writer left alone)
    with pytest.raises(st.SurrogateTrainError, match="no file"):
        st.init_domain(str(tmp_path / "nothing"), n_in)


def test_loader_refusals(mw, tmp_path):
    from miniweatherml_amd import modules
    p = tmp_path / "training_domain.txt"
    good = "".join("%r %r\n" % (float(lo), float(hi)) for lo, hi in SINGLE)
    p.write_text(good)
    assert np.array_equal(modules.load_training_domain(str(p), 5), SINGLE)
    for text, n_in, msg in ((good, 9, "9 rows"), (good + "0.0 1.0\n", 5, "5 rows"), (good.replace("320.0", "nan"), 5, "NaN"),
                            (good.replace("200.0 320.0", "320.0 200.0"), 5, "row 0 has min > max"), (good.replace(" ", " 1.0 "), 5, "5 rows"),
                            ("", 5, "5 rows"), (good.replace("320.0", "high"), 5, "training_domain.txt")):
        p.write_text(text)
        with pytest.raises(modules.MWError, match=msg) as err:
            modules.load_training_domain(str(p), n_in)
        assert str(p) in str(err.value)                                        # the file is named
    with pytest.raises(modules.MWError, match="nowhere.txt"):
        modules.load_training_domain(str(tmp_path / "nowhere.txt"), 5)


# ---- domain_box(..., tables=) -----------------------------------------------------------------------------------------------------------------
def test_domain_box_with_tables():
    from miniweatherml_amd import modules
    wide = SINGLE.copy()
    wide[0] = [180.0, 350.0]
    wide[4, 1] = 9.0e-3
    for m in (0.0, 0.05):
        plain = modules.domain_box([model(SINGLE)], m, names=["a"])
        assert np.array_equal(bits(modules.domain_box([model(SINGLE)], m, names=["a"], tables=None)), bits(plain))
        assert np.array_equal(bits(modules.domain_box([model(SINGLE)], m, names=["a"], tables=[None])), bits(plain))      # today's box, bit for bit
        got = modules.domain_box([model(SINGLE)], m, names=["a"], tables=[wide])
        w = wide[:, 1] - wide[:, 0]
        want = np.stack([wide[:, 0] - np.float64(m) * w, wide[:, 1] + np.float64(m) * w], axis=1)       # the margin on the TABLE's width
        assert np.array_equal(bits(got), bits(want))
        assert got[0, 0] < plain[0, 0] and got[0, 1] > plain[0, 1] and got[4, 1] > plain[4, 1] and np.array_equal(bits(got[1:4]), bits(plain[1:4]))
    narrow = SINGLE.copy()
    narrow[2] = [0.005, 0.01]
    assert np.array_equal(bits(modules.domain_box([model(SINGLE)], tables=[narrow])), bits(narrow))      # narrower than the rows: it is data
    # the stencil model's intersection is taken from the table's rows, not from the scaling rows
    tab9 = STENCIL.copy()
    tab9[0], tab9[5] = [150.0, 340.0], [160.0, 335.0]
    got = modules.domain_box([model(STENCIL)], tables=[tab9])
    assert got[0].tolist() == [160.0, 335.0] and modules.domain_box([model(STENCIL)])[0].tolist() == [210.0, 320.0]
    assert np.array_equal(bits(got[1:]), bits(modules.domain_box([model(STENCIL)])[1:]))
    # a committee of a model with a table and one without: the intersection of the table and the other's rows
    other = SINGLE.copy()
    other[0] = [190.0, 330.0]
    both = modules.domain_box([model(SINGLE), model(other)], tables=[wide, None])
    assert both[0].tolist() == [190.0, 330.0] and both[4].tolist() == [0.0, 7.0e-3]
    assert modules.domain_box([model(SINGLE), model(other)])[0].tolist() == [200.0, 320.0]
    for tables, msg in (([wide, None, None], "2 models"), ([STENCIL, None], r"\(9, 2\)")):
        with pytest.raises(ValueError, match=msg):
            modules.domain_box([model(SINGLE), model(other)], tables=tables)


def test_rollout_hands_its_domains_to_every_box():
    """Microphysics_Rollout with hand-set models: the report's boxes and a committee's box read the tables."""
    from miniweatherml_amd import modules
    wide = SINGLE.copy()
    wide[0] = [100.0, 400.0]
    micro = modules.Microphysics_Rollout.__new__(modules.Microphysics_Rollout)
    micro._models, micro._model_names, micro._committee_names = [model(SINGLE), model(SINGLE)], ["a", "b"], [("both", ["a", "b"]), ("solo", ["a"])]
    micro.member_names = ["kessler", "a", "b", "both", "solo"]
    micro._domain, micro._domain_counts, micro._domain_steps, micro._domain_cells = None, None, [], (96, 12)
    micro._domains = [wide, None]
    micro.training_domain = True
    _, members, boxes = micro._domain_setup()
    assert members == [1, 2, 3, 4]
    assert boxes[0][0].tolist() == [100.0, 400.0] and boxes[1][0].tolist() == [200.0, 320.0]
    assert boxes[2][0].tolist() == [200.0, 320.0] and boxes[3][0].tolist() == [100.0, 400.0]
    assert micro.model_box("a", 0.5)[0].tolist() == [-50.0, 550.0] and micro.model_box("b")[0].tolist() == [200.0, 320.0]


# ---- nn_training_domain ---------------------------------------------------------------------------------------------------------------------
def test_surrogate_models_take_the_optional_key(mw, tmp_path):
    from miniweatherml_amd import driver, modules, surrogate_train as st
    _, models = model_list(tmp_path, 2)
    entry = dict(models[0])
    assert driver._surrogate_models([dict(entry)], str(tmp_path)) == [entry]                             # absent: the entry is what it was
    table = st.write_training_domain(str(tmp_path / "t"), modules.load_surrogate_weights()[4])
    got = driver._surrogate_models([dict(entry, nn_training_domain=table), dict(models[1])], str(tmp_path))
    assert got == [dict(entry, nn_training_domain=table), models[1]]
    rel = driver._surrogate_models([dict(entry, nn_training_domain=os.path.join("t", "training_domain.txt"))], str(tmp_path))
    assert rel[0]["nn_training_domain"] == table                                                         # resolved from the YAML's directory
    with pytest.raises(FileNotFoundError, match=r"no file .*missing\.txt"):
        driver._surrogate_models([dict(entry, nn_training_domain="missing.txt")], str(tmp_path))
    bank = modules.load_surrogate_bank(got)
    tabs = modules.load_training_domains(got, bank)
    assert tabs[1] is None and np.array_equal(bits(tabs[0]), bits(bank[0].scl_in))
    assert len(bank[0]) == 7                                                                             # the tuple has no new field


# ---- the report -----------------------------------------------------------------------------------------------------------------------------
def test_report_blocks_from_hand_made_counts():
    from miniweatherml_amd import modules
    cfg = {"share": 0.5, "margin": 0.0, "fields": list(IN5)}
    box = SINGLE.copy()
    box[1] = [-math.inf, math.inf]
    taken = {"a": {"outside": 3, "active": 20, "inactive": 27}, "b": {"outside": 0, "active": 0, "inactive": 0}}
    eligible = {"a": {"outside": 3, "active": 400, "inactive": 600}, "b": {"outside": 0, "active": 1, "inactive": 999}}
    rep = modules.harvest_outside_report(cfg, ["a", "b"], [box, SINGLE], taken, eligible)
    assert sorted(rep) == ["eligible", "outside", "taken"]
    assert rep["outside"]["share"] == 0.5 and rep["outside"]["margin"] == 0.0 and rep["outside"]["fields"] == list(IN5)
    assert rep["outside"]["boxes"]["a"]["temp"] == [200.0, 320.0] and rep["outside"]["boxes"]["a"]["density_dry"] == ["-inf", "inf"]
    assert rep["outside"]["boxes"]["b"] == modules.box_json(SINGLE)
    assert rep["taken"] == taken and rep["eligible"] == eligible
    json.dumps(rep, allow_nan=False)
    assert modules.SAMPLE_CLASSES == ref.CLASSES
    # the document's block, from stand-in harvesters: with the option the three blocks, without it exactly the keys it always had
    from types import SimpleNamespace
    from miniweatherml_amd import driver
    harvest = {"interval": 2, "samples_per_step": 50, "ratio_active": 0.5, "seed": 1, "max_rainsplit": 64, "members": ["a", "b"]}
    base = dict(files={"a": "fa", "b": "fb"}, samples={"a": 50, "b": 0}, skipped={"a": 0, "b": 1}, calls=1, member_names=["a", "b"])
    plain = driver.harvest_block(harvest, SimpleNamespace(outside=None, **base))
    assert plain == dict(harvest, files=base["files"], samples=base["samples"], skipped=base["skipped"], calls=1)
    assert list(plain) == list(harvest) + ["files", "samples", "skipped", "calls"]
    assert not {"outside", "taken", "eligible"} & set(plain)
    full = driver.harvest_block(dict(harvest, outside=cfg), SimpleNamespace(outside=cfg, boxes=[box, SINGLE], taken=taken, eligible=eligible, **base))
    assert {k: full[k] for k in plain} == plain and {k: full[k] for k in rep} == rep and set(full) == set(plain) | set(rep)
    json.dumps(full, allow_nan=False)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_exports_agree(mw):
    from miniweatherml_amd import capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mw_cdna4.h")).read(), flags=re.S)
    m = re.search(r"\bmw_member_sample_mask_domain\s*\(([^)]*)\)", header)
    assert m and len(m.group(1).split(",")) == 14
    assert len(capi.SYMBOLS["mw_member_sample_mask_domain"][1]) == 14 and hasattr(C.CDLL(capi.LIB_PATH), "mw_member_sample_mask_domain")
    assert capi.MW_SAMPLE_CLASSES == 3 and capi.MW_SAMPLE_WORDS == 6


def call_mask(L, mask, counts, nz=4, ncol=16, nens=3, members=(2, 0), box=Ellipsis, above=Ellipsis, thr=Ellipsis, fields=Ellipsis,
              teacher=Ellipsis):
    """mw_member_sample_mask_domain with made-up field addresses; mask / counts: host numpy arrays or None."""
    nm = 0 if members is None else len(members)
    if box is Ellipsis:
        box = np.tile(np.array([[-1.0, 1.0]]), (max(1, nm), 5, 1))
    if thr is Ellipsis:
        thr = np.full((max(1, nm), 3), 0.5)
    if above is Ellipsis:
        above = [0] * max(1, nm)
    f5 = (C.c_void_p * 5)(*[0x1000] * 5) if fields is Ellipsis else fields
    t4 = (C.c_void_p * 4)(*[0x2000] * 4) if teacher is Ellipsis else teacher
    dbl = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))     # noqa: E731
    return L.mw_member_sample_mask_domain(nz, ncol, nens, nm, None if members is None else (C.c_int * max(1, nm))(*members), dbl(box),
                                          None if above is None else (C.c_int * len(above))(*above), f5, t4, 12345, dbl(thr),
                                          None if mask is None else C.c_void_p(mask.ctypes.data),
                                          None if counts is None else C.c_void_p(counts.ctypes.data), None)


def test_argument_refusals_come_before_the_device_check(mw):
    """The fields are made-up addresses, mask and counts sentinel-filled host arrays: no call below may reach the device or write them."""
    import torch
    from miniweatherml_amd import capi
    L = capi.lib()
    mask, counts = np.full(4 * 16 * 3, 7, dtype=np.uint8), np.full((2, 6), -99, dtype=np.int64)

    def box(at, value):
        b = np.tile(np.array([[-1.0, 1.0]]), (2, 5, 1))
        b[at] = value
        return b

    def thr(at, value):
        t = np.full((2, 3), 0.5)
        t[at] = value
        return t
    hole5 = (C.c_void_p * 5)(0x1000, 0x1000, None, 0x1000, 0x1000)
    hole4 = (C.c_void_p * 4)(0x2000, None, 0x2000, 0x2000)
    cases = [(dict(fields=None), b"null pointer"), (dict(teacher=None), b"null pointer"), (dict(fields=hole5), b"null field"),
             (dict(teacher=hole4), b"null field"), (dict(members=None), b"null pointer"), (dict(box=None), b"null pointer"),
             (dict(above=None), b"null pointer"), (dict(thr=None), b"null pointer"), (dict(nz=0), b"must be >= 1"), (dict(ncol=0), b"must be >= 1"),
             (dict(nens=0), b"nens must be"), (dict(nens=65), b"nens must be"), (dict(members=[]), b"nm must be"),
             (dict(nens=64, members=list(range(33))), b"nm must be"), (dict(members=[1, 1]), b"listed twice"),
             (dict(members=[0, 3]), b"outside [0, 3)"), (dict(members=[-1, 0]), b"outside [0, 3)"),
             (dict(box=box((1, 2, 0), 2.0)), b"not lo <= hi"), (dict(box=box((0, 4, 1), math.nan)), b"not lo <= hi"),
             (dict(box=box((0, 0, 0), math.nan)), b"not lo <= hi"), (dict(thr=thr((0, 0), math.nan)), b"NaN or outside [0, 1]"),
             (dict(thr=thr((1, 2), 1.5)), b"NaN or outside [0, 1]"), (dict(thr=thr((1, 1), -1.0e-300)), b"NaN or outside [0, 1]"),
             (dict(thr=thr((0, 1), math.inf)), b"NaN or outside [0, 1]")]
    for kw, msg in cases:
        assert call_mask(L, mask, counts, **kw) != 0 and msg in L.mw_last_error(), kw
    assert call_mask(L, mask, None) != 0 and b"null pointer (counts" in L.mw_last_error()
    assert call_mask(L, None, None) != 0 and b"null pointer (counts" in L.mw_last_error()
    inf_box = np.tile(np.array([[-math.inf, math.inf]]), (2, 5, 1))
    if not torch.cuda.is_available():                                          # valid calls: an infinite box, thresholds 0 and 1, no mask
        assert call_mask(L, mask, counts, box=inf_box, thr=np.array([[0.0, 1.0, 0.5]] * 2)) != 0 and b"no HIP device" in L.mw_last_error()
        assert call_mask(L, None, counts) != 0 and b"no HIP device" in L.mw_last_error()
    assert (mask == 7).all() and (counts == -99).all()
