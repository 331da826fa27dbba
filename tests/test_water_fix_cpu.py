"""The water fixer without a GPU: the numpy statement of the rule (water_fix_ref.py) against its own properties, the
`water_fixer:` key's checks, and the report builder from raw arrays."""
import json

import numpy as np
import pytest

import water_fix_ref as ref


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def state(nz, ncol, nens, seed):
    """Non-negative fields before and after a step in which about half the columns gain water."""
    rng = np.random.default_rng(seed)
    before = [rng.uniform(0.0, hi, (nz, ncol, nens)) for hi in (2.0e-2, 2.0e-3, 5.0e-3)]
    factor = rng.uniform(0.5, 1.5, (ncol, nens))
    after = [q * factor * rng.uniform(0.99, 1.01, q.shape) for q in before]
    return before, after


@pytest.mark.parametrize("nz,ncol,nens,dz", [(1, 5, 1, 500.0), (4, 70, 3, 150.0), (37, 300, 2, 500.0), (100, 64, 4, 200.0)])
def test_reference_properties(nz, ncol, nens, dz):
    before, after = state(nz, ncol, nens, seed=nz + ncol)
    wb = ref.column_water(*before, dz)
    precl0, total0 = np.full((ncol, nens), -3.0), np.full((ncol, nens), 0.25)
    fixed = list(range(nens))[-2:]
    members = list(range(nens))
    out = ref.water_fix(*after, dz, 60.0, wb, precl0, total0, members, members, fixed)
    fix = out["fixed"]
    assert fix.any() and not fix.all() and not out["skipped"].any()
    assert not fix[:, [m for m in members if m not in fixed]].any()
    # the bound, and precl of a fixed column is the residual's
    w_now = ref.column_water(out["v"], out["c"], out["r"], dz)
    assert same_bits(w_now, out["w_now"])
    assert np.all(np.abs(w_now[fix] - wb[fix]) <= ref.bound(nz, wb[fix]))
    assert same_bits(out["precl"], (wb - w_now) / (1000.0 * 60.0))
    assert np.all(np.abs(out["precl"][fix]) <= ref.bound(nz, wb[fix]) / 60000.0)
    assert same_bits(out["rain_total"], total0 + 60.0 * out["precl"])
    # unfixed columns: untouched to the bit, today's precl
    for got, was in zip((out["v"], out["c"], out["r"]), after):
        assert same_bits(got[:, ~fix], was[:, ~fix]) and not np.array_equal(got[:, fix], was[:, fix])
    assert same_bits(out["precl"][~fix], ((wb - out["w_after"]) / 60000.0)[~fix])
    assert np.all(out["excess"][fix] > 0.0) and np.all(bits(out["excess"][~fix]) == 0)
    assert np.array_equal(out["counts"][:, 0], fix.sum(axis=0)) and np.all(out["counts"][:, 1] == 0)
    # signs and zeros are kept
    assert np.all(out["v"] >= 0.0)
    # a second application finds at most rounding-size excess
    again = ref.water_fix(out["v"], out["c"], out["r"], dz, 60.0, wb, precl0, total0, members, members, fixed)
    assert np.all(again["excess"] <= ref.bound(nz, wb))
    assert not again["fixed"][~fix].any()
    # ... and none at all with a tolerance above it
    calm = ref.water_fix(out["v"], out["c"], out["r"], dz, 60.0, wb, precl0, total0, members, members, fixed, tolerance=(nz + 4) * 2.0 ** -52)
    assert not calm["fixed"].any() and all(same_bits(calm[k], out[k]) for k in "vcr")


def test_reference_skips_and_edges():
    nz, ncol, nens, dz = 5, 12, 2, 100.0
    before, after = state(nz, ncol, nens, seed=3)
    for q in after:
        q[:] = q * 2.0                                                          # every column gains
    wb = ref.column_water(*before, dz)
    after[1][2, 0, 1] = np.nan
    after[2][4, 1, 1] = np.inf
    wb[2, 1] = np.nan
    wb[3, 1] = -1.0                                                             # negative before-water, W_a > W_b
    wb[4, 1] = 0.0                                                              # W_b = 0 with W_a > 0: every water field becomes 0
    for q, b in zip(after, before):                                             # W_a == W_b exactly
        q[:, 5, 1] = b[:, 5, 1]
    wb[5, 1] = ref.column_water(*[q[:, 5:6, 1:2] for q in after], dz)[0, 0]
    precl0, total0 = np.full((ncol, nens), -3.0), np.zeros((ncol, nens))
    out = ref.water_fix(*after, dz, 1.0, wb, precl0, total0, [0, 1], [0, 1], [1])
    assert list(np.flatnonzero(out["skipped"][:, 1])) == [0, 1, 2, 3] and not out["skipped"][:, 0].any()
    assert out["counts"].tolist() == [[0, 0], [ncol - 5, 4]]
    for got, was in zip((out["v"], out["c"], out["r"]), after):
        assert same_bits(got[:, :4], was[:, :4]) and same_bits(got[:, 5], was[:, 5]) and same_bits(got[..., 0], was[..., 0])
    assert np.isnan(out["precl"][0, 1]) and out["precl"][1, 1] == -np.inf and np.isnan(out["precl"][2, 1])
    assert all(np.all(out[k][:, 4, 1] == 0.0) for k in "vcr") and out["fixed"][4, 1] and out["precl"][4, 1] == 0.0
    assert not out["fixed"][5, 1] and bits(out["precl"][5, 1]) == 0
    # the tolerance edge in powers of two: W_b = 1, W_a = 1.5
    one = [np.full((1, 1, 1), x) for x in (1.0, 0.25, 0.25)]
    args = (1.0, 1.0, np.ones((1, 1)), np.zeros((1, 1)), np.zeros((1, 1)), [0], [0], [0])
    assert not ref.water_fix(*one, *args, tolerance=0.5)["fixed"].any()
    edge = ref.water_fix(*one, *args, tolerance=np.nextafter(0.5, 0.0))
    assert edge["fixed"].all() and edge["excess"][0, 0] == 0.5


def test_water_fixer_config():
    from miniweatherml_amd import driver
    names = ["tend0", "mean3"]
    assert driver.water_fixer_config({}) is None and driver.water_fixer_config({"water_fixer": False}) is None
    assert driver.water_fixer_config({"water_fixer": None}) is None
    assert driver.water_fixer_config({"water_fixer": True}, names) == {"members": None, "tolerance": 0.0}
    assert driver.water_fixer_config({"water_fixer": {}}, names) == {"members": None, "tolerance": 0.0}
    got = driver.water_fixer_config({"water_fixer": {"members": ["mean3"], "tolerance": 1}}, names)
    assert got == {"members": ["mean3"], "tolerance": 1.0} and type(got["tolerance"]) is float
    assert driver.water_fixer_config({"water_fixer": {"members": ["anything"]}})["members"] == ["anything"]     # (no names to check against)
    for bad, msg in ((3, "true, false or a mapping"), ("yes", "true, false or a mapping"), ([1], "true, false or a mapping"),
                     ({"member": ["tend0"]}, r"unknown key\(s\) 'member' in water_fixer"), ({"tolerance": -1.0e-9}, "finite number >= 0"),
                     ({"tolerance": float("nan")}, "finite number >= 0"), ({"tolerance": float("inf")}, "finite number >= 0"),
                     ({"tolerance": "0"}, "finite number >= 0"), ({"tolerance": True}, "finite number >= 0"),
                     ({"members": []}, "non-empty list"), ({"members": "tend0"}, "non-empty list"), ({"members": ["tend0", "tend0"]}, "non-empty list"),
                     ({"members": [1]}, "non-empty list"), ({"members": ["kessler"]}, "only a member that a network steps"),
                     ({"members": ["tend0", "persistence"]}, "only a member that a network steps"),
                     ({"members": ["nobody"]}, "no model or committee of this run")):
        with pytest.raises(ValueError, match=msg):
            driver.water_fixer_config({"water_fixer": bad}, names)


def test_load_config_keeps_the_key(tmp_path):
    from miniweatherml_amd import driver
    base = ("sim_time: 1\nnx_glob: 4\nny_glob: 4\nnz: 4\nxlen: 1\nylen: 1\nzlen: 1\ndt_phys: 1\nout_prefix: t\ninit_data: supercell\n"
            "out_freq: 1\n")
    p = tmp_path / "a.yaml"
    p.write_text(base + "water_fixer: {members: [a], tolerance: 0.5}\n")
    assert driver.load_config(str(p))["water_fixer"] == {"members": ["a"], "tolerance": 0.5}
    p.write_text(base)
    assert "water_fixer" not in driver.load_config(str(p))


def test_report_from_raw_arrays():
    from miniweatherml_amd import modules
    names = ["kessler", "a", "b", "persistence"]
    z = np.zeros((4, 2))
    c0, s0 = z.astype(np.int64), z.copy()
    c0[1], s0[1] = [3, 1], [1.5, 1.0]
    c0[2], s0[2] = [9, 9], [9.0, 9.0]                                           # (member b is not fixed: never shown)
    c1, s1 = z.astype(np.int64), z.copy()
    c1[1], s1[1] = [2, 0], [0.5, 0.25]
    doc = modules.water_fix_report(names, [1], 0.0, 10, [(0, c0, s0), (5, c1, s1)])
    assert doc == json.loads(json.dumps(doc, allow_nan=False))
    assert doc["tolerance"] == 0.0 and doc["members"] == ["a"] and doc["columns"] == 10 and [s["step"] for s in doc["steps"]] == [0, 5]
    assert doc["steps"][0]["members"] == {"a": {"columns_fixed": 3, "columns_skipped": 1, "water_removed_kg_m2": {"mean": 0.15, "max": 1.0}}}
    assert doc["steps"][1]["members"]["a"]["water_removed_kg_m2"] == {"mean": 0.05, "max": 0.25}
    assert doc["totals"] == {"a": {"columns_fixed": 5, "columns_skipped": 1, "water_removed_kg_m2": {"mean": 0.15 + 0.05, "max": 1.0}}}
    empty = modules.water_fix_report(names, [1, 2], 1.0e-12, 10, [])
    assert empty["steps"] == [] and empty["members"] == ["a", "b"] and empty["totals"]["b"]["columns_fixed"] == 0
    with pytest.raises(modules.MWError, match="counts and"):
        modules.water_fix_report(names, [1], 0.0, 10, [(0, c0[:3], s0)])
    with pytest.raises(modules.MWError, match="distinct indices"):
        modules.water_fix_report(names, [1, 1], 0.0, 10, [])
