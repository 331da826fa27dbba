"""The surface-rain reports without a GPU: rain_scores' arithmetic from hand-made counts with every zero denominator, rain_report's units
(m / s to mm / h, m to mm), its JSON with non-finite statistics present, RainScorer's pure part, and the `surface_rain:` block's checks."""
import json

import numpy as np
import pytest

MEMBERS = ["kessler", "net", "persistence"]


def test_scores_from_hand_made_counts():
    from miniweatherml_amd import modules
    assert modules.RAIN_COUNTS == ("hits", "misses", "false_alarms", "correct_negatives", "nonfinite")
    r = modules.rain_scores([6, 2, 4, 87, 1])
    assert [r[k] for k in modules.RAIN_COUNTS] == [6, 2, 4, 87, 1]
    assert r["csi"] == 6 / 12 and r["pod"] == 6 / 8 and r["far"] == 4 / 10 and r["frequency_bias"] == 10 / 8
    # nothing observed, nothing forecast: every denominator is 0
    r = modules.rain_scores([0, 0, 0, 50, 0])
    assert r["csi"] is None and r["pod"] is None and r["far"] is None and r["frequency_bias"] is None
    # forecast only: h + m = 0 (pod and the frequency bias), the others defined
    r = modules.rain_scores([0, 0, 3, 47, 0])
    assert r["csi"] == 0.0 and r["pod"] is None and r["far"] == 1.0 and r["frequency_bias"] is None
    # observed only: h + f = 0 (far)
    r = modules.rain_scores([0, 5, 0, 45, 0])
    assert r["csi"] == 0.0 and r["pod"] == 0.0 and r["far"] is None and r["frequency_bias"] == 0.0
    # a perfect member
    r = modules.rain_scores([7, 0, 0, 43, 0])
    assert r["csi"] == 1.0 and r["pod"] == 1.0 and r["far"] == 0.0 and r["frequency_bias"] == 1.0
    assert all(type(r[k]) is int for k in modules.RAIN_COUNTS)


def raw(ncol, thr_rate, thr_acc, seed=0):
    """Host fields (ncol, 3) of a rate in m / s and an accumulation in m, and member_divergence's / member_rain_table's arrays of them."""
    rng = np.random.default_rng(seed)
    rate = rng.uniform(0.0, 1.0e-5, (ncol, 3))                                 # up to 36 mm / h
    acc = rng.uniform(0.0, 3.0e-2, (ncol, 3))                                  # up to 30 mm
    stats, tables = np.zeros((3, 2, 7)), []
    for f, (x, thr, unit) in enumerate(((rate, thr_rate, 3.6e6), (acc, thr_acc, 1.0e3))):
        d = x - x[:, :1]
        stats[:, f] = np.stack([d.sum(0), np.abs(d).sum(0), (d * d).sum(0), np.abs(d).max(0), x.sum(0), x.min(0), x.max(0)], axis=1)
        t = np.zeros((len(thr), 3, 5), dtype=np.int64)
        for j, q in enumerate(thr):
            fc, ob = x >= q / unit, x[:, :1] >= q / unit
            t[j, :, 0], t[j, :, 1], t[j, :, 2], t[j, :, 3] = (fc & ob).sum(0), (~fc & ob).sum(0), (fc & ~ob).sum(0), (~fc & ~ob).sum(0)
        tables.append(t)
    return rate, acc, stats, np.zeros((3, 2), dtype=np.int64), tables


def test_report_units_and_layout():
    from miniweatherml_amd import modules
    thr_rate, thr_acc = [0.1, 5.0, 25.0], [1.0, 10.0]
    ncol = 40
    rate, acc, stats, nonf, tables = raw(ncol, thr_rate, thr_acc)
    rep = modules.rain_report(stats, nonf, tables, ncol, MEMBERS, thr_rate, thr_acc)
    assert list(rep) == MEMBERS and all(tuple(rep[m]) == modules.RAIN_FIELDS == ("rate_mm_h", "accumulation_mm") for m in MEMBERS)
    for m, name in enumerate(MEMBERS):
        for x, fname, unit, thr in ((rate, "rate_mm_h", 3.6e6, thr_rate), (acc, "accumulation_mm", 1.0e3, thr_acc)):
            row = rep[name][fname]
            d = unit * (x[:, m] - x[:, 0])
            want = {"bias": d.mean(), "mae": np.abs(d).mean(), "rmse": np.sqrt((d * d).mean()), "max_abs": np.abs(d).max(),
                    "mean": unit * x[:, m].mean(), "min": unit * x[:, m].min(), "max": unit * x[:, m].max()}
            for k, v in want.items():
                assert row[k] == pytest.approx(v, rel=1e-12, abs=1e-300), (name, fname, k)
            assert row["nonfinite"] == 0 and "finite" not in row
            assert [t["threshold"] for t in row["thresholds"]] == thr
            for t in row["thresholds"]:
                assert t["hits"] + t["misses"] + t["false_alarms"] + t["correct_negatives"] + t["nonfinite"] == ncol
    # one metre per second is 3.6e6 mm / h, one metre 1000 mm: a member that rains exactly that everywhere
    one = np.zeros((3, 2, 7))
    one[1, :, 4:] = [[ncol, 1.0, 1.0]] * 2
    z = [np.zeros((1, 3, 5), dtype=np.int64)] * 2
    rep = modules.rain_report(one, nonf, z, ncol, MEMBERS, [1.0], [1.0])
    assert rep["net"]["rate_mm_h"]["mean"] == 3.6e6 and rep["net"]["rate_mm_h"]["max"] == 3.6e6
    assert rep["net"]["accumulation_mm"]["mean"] == 1000.0 and rep["net"]["accumulation_mm"]["min"] == 1000.0
    # the Kessler member against itself
    rep = modules.rain_report(stats, nonf, tables, ncol, MEMBERS, thr_rate, thr_acc)
    k = rep["kessler"]["rate_mm_h"]
    assert k["bias"] == 0.0 and k["rmse"] == 0.0 and all(t["misses"] == 0 and t["false_alarms"] == 0 for t in k["thresholds"])


def test_report_with_non_finite_statistics_is_json():
    from miniweatherml_amd import modules
    thr = [1.0, 10.0]
    ncol = 25
    _, _, stats, nonf, tables = raw(ncol, thr, thr, seed=2)
    stats[1, 0, :] = [np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan]   # a NaN column of the net's rate
    stats[1, 1, :] = [np.inf, np.inf, np.inf, np.inf, np.inf, 0.0, np.inf]      # an inf column of its accumulation
    nonf[1] = [1, 1]
    for t in tables:
        t[:, 1, 3] -= 1
        t[:, 1, 4] += 1
    scorer = modules.RainScorer(MEMBERS, thr, thr)
    scorer.add(stats, nonf, tables, ncol, 4, 12.5)
    rep = scorer.report()
    text = json.dumps(rep, allow_nan=False)
    back = json.loads(text)
    assert back["thresholds_mm_h"] == thr and back["thresholds_mm"] == thr and [t["step"] for t in back["times"]] == [4]
    net = back["times"][0]["members"]["net"]
    assert net["rate_mm_h"]["finite"] is False and all(net["rate_mm_h"][k] is None for k in ("bias", "mae", "rmse", "max_abs", "mean", "min", "max"))
    assert net["accumulation_mm"]["finite"] is False and net["accumulation_mm"]["min"] == 0.0 and net["accumulation_mm"]["max"] is None
    assert net["rate_mm_h"]["nonfinite"] == 1 and net["rate_mm_h"]["thresholds"][0]["nonfinite"] == 1
    assert "finite" not in back["times"][0]["members"]["persistence"]["rate_mm_h"]
    assert "persistence" in scorer.table() and len(scorer.table().split("\n")) == 2 + len(MEMBERS)


def test_report_refuses_arrays_of_the_wrong_shape():
    from miniweatherml_amd import modules
    _, _, stats, nonf, tables = raw(10, [1.0], [1.0])
    with pytest.raises(modules.MWError, match="rain_report"):
        modules.rain_report(stats, nonf, tables, 10, MEMBERS[:2], [1.0], [1.0])
    with pytest.raises(modules.MWError, match="rain_report"):
        modules.rain_report(stats, nonf, tables, 10, MEMBERS, [1.0, 2.0], [1.0])
    with pytest.raises(modules.MWError, match="nothing accumulated"):
        modules.RainScorer(MEMBERS).report()


def test_surface_rain_block_of_the_configuration():
    from miniweatherml_amd import driver
    default = [0.1, 1.0, 5.0, 10.0, 25.0]
    assert driver.surface_rain_config({}) is None and driver.surface_rain_config({"surface_rain": False}) is None
    assert driver.surface_rain_config({"surface_rain": True}) == {"thresholds_mm_h": default, "thresholds_mm": default, "map": True}
    got = driver.surface_rain_config({"surface_rain": {"thresholds_mm": [2, 4.5], "map": False}})
    assert got == {"thresholds_mm_h": default, "thresholds_mm": [2.0, 4.5], "map": False}
    eight = [1, 2, 3, 4, 5, 6, 7, 8]
    assert driver.surface_rain_config({"surface_rain": {"thresholds_mm_h": eight}})["thresholds_mm_h"] == [float(x) for x in eight]
    for block, msg in (({"threshold_mm": [1.0]}, "unknown key"),
                       ({"thresholds_mm_h": [1.0, 0.5]}, "strictly ascending"),
                       ({"thresholds_mm": [1.0, 1.0]}, "strictly ascending"),
                       ({"thresholds_mm": [0.0, 1.0]}, "positive"),
                       ({"thresholds_mm_h": [-1.0]}, "positive"),
                       ({"thresholds_mm_h": [float("nan")]}, "positive"),
                       ({"thresholds_mm": eight + [9]}, "1 to 8"),
                       ({"thresholds_mm": []}, "1 to 8"),
                       ({"thresholds_mm": 5.0}, "1 to 8"),
                       ({"thresholds_mm": [True]}, "positive"),
                       ({"map": 1}, "map must be true or false"),
                       ({"map": "yes"}, "map must be true or false"),
                       ("on", "true, false or a mapping")):
        with pytest.raises(ValueError, match=msg):
            driver.surface_rain_config({"surface_rain": block})


def test_load_config_hands_the_block_on(tmp_path):
    from miniweatherml_amd import driver
    p = tmp_path / "in.yaml"
    base = ("sim_time: 1\nnx_glob: 4\nny_glob: 4\nnz: 4\nxlen: 1\nylen: 1\nzlen: 1\ndt_phys: 0\nout_prefix: o\ninit_data: supercell\n"
            "out_freq: -1\n")
    p.write_text(base + "surface_rain: {thresholds_mm_h: [0.5, 2], map: false}\n")
    assert driver.surface_rain_config(driver.load_config(str(p))) == {"thresholds_mm_h": [0.5, 2.0],
                                                                      "thresholds_mm": [0.1, 1.0, 5.0, 10.0, 25.0], "map": False}
    p.write_text(base)
    cfg = driver.load_config(str(p))
    assert "surface_rain" not in cfg and driver.surface_rain_config(cfg) is None
