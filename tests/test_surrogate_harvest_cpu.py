"""Harvesting Kessler labels on the rollout members' own states, without a GPU: the teacher's decision function (the only thing that sizes
its sub-cycle loop), the `harvest:` block of the rollout_surrogates YAML, the trainer's warm start as far as the host goes, and the host
statement of the sample masks' draw that the GPU test uses."""
import ctypes as C
import math
import os
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = "sim_time: 10\nnx_glob: 8\nny_glob: 8\nnz: 8\nxlen: 1\nylen: 1\nzlen: 1\ndt_phys: 0\nout_prefix: x\ninit_data: supercell\nout_freq: -1\n"
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- the draw: numpy restatement of u01_from_key (csrc/mw_sample_key.h) ----------------------------------------------------------------
def u01(keys):
    """splitmix64's finaliser of uint64 keys (wrapping arithmetic), the top 53 bits as a double in [0, 1)."""
    with np.errstate(over="ignore"):
        z = np.asarray(keys, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def test_u01_host_statement_is_pinned():
    """Three keys computed by hand with Python integers (splitmix64 of 0 is the generator's published first output 0xE220A8397B1DCDAF),
    one of them near 2^64 so that the key addition wraps."""
    def by_hand(k):
        m = (1 << 64) - 1
        z = (k + 0x9E3779B97F4A7C15) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        z ^= z >> 31
        return z
    assert by_hand(0) == 0xE220A8397B1DCDAF
    keys = [0, 12345678901234567, (1 << 64) - 3]
    want = [(by_hand(k) >> 11) / 9007199254740992.0 for k in keys]
    got = u01(np.array(keys, dtype=np.uint64))
    assert got.tolist() == want
    assert want[0] == 0xE220A8397B1DCDAF // 2048 / 2.0 ** 53 and all(0.0 <= x < 1.0 for x in want)
    from miniweatherml_amd import surrogate_train as st
    assert [st.splitmix64(k) for k in keys] == [by_hand(k) for k in keys]          # (the trainer's Python statement of the same finaliser)


# ---- the decision function ------------------------------------------------------------------------------------------------------------
def test_teacher_rainsplit_decision(mw):
    from miniweatherml_amd import capi
    f = capi.lib().mw_kessler_teacher_rainsplit
    dt = 300.0
    assert f(dt, dt, 64) == 1
    assert f(dt, dt / 3.5, 64) == 4
    assert f(dt, 2.0 * dt, 64) == 1                                  # (a word above dt: the kernels cap it at dt anyway)
    assert f(dt, dt / 64.0, 64) == 64                                # a count equal to the cap
    assert f(dt, dt / 65.0, 64) == 0                                 # cap + 1
    assert f(dt, dt / 64.5, 64) == 0                                 # ceil = 65
    assert f(dt, dt / 1024.0, 1024) == 1024 and f(dt, dt / 1025.0, 1024) == 0
    assert f(dt, dt / 3.5, 4) == 4 and f(dt, dt / 3.5, 3) == 0
    t0 = time.perf_counter()
    for bad in (0.0, -0.0, -1.0, 5e-324, 2.2e-308, 1e-300, math.inf, -math.inf, math.nan):
        assert f(dt, bad, 64) == 0, bad
        assert f(dt, bad, 1024) == 0, bad
    assert time.perf_counter() - t0 < 1.0                            # decided, not counted towards


def test_new_entry_points_fail_loudly_without_gpu(mw):
    import torch
    from miniweatherml_amd import capi
    L = capi.lib()
    assert L.mw_kessler_members_teacher_workspace_bytes(10, 100, 3) == 512 + 8 * (10 + 2 + 1) * 300
    assert L.mw_kessler_members_teacher_workspace_bytes(1, 100, 3) == 0 and L.mw_kessler_members_teacher_workspace_bytes(10, 100, 65) == 0
    f5 = (C.c_void_p * 5)(*[0x1000] * 5)
    o4 = (C.c_void_p * 4)(*[0x2000] * 4)
    ws = C.c_void_p(0x3000)

    def teacher(nz=4, ncol=16, nens=3, members=(1, 2), dt=1.0, cap=64, fields=f5, outs=o4, work=ws):
        return L.mw_kessler_members_teacher(nz, ncol, nens, len(members), (C.c_int * max(1, len(members)))(*members), 500.0, dt, cap, fields, outs,
                                            None, work, None)
    for kw, msg in ((dict(nz=1), b"nz >= 2"), (dict(members=(1, 3)), b"outside [0, 3)"), (dict(members=(-1,)), b"outside [0, 3)"),
                    (dict(members=(2, 2)), b"listed twice"), (dict(members=()), b"nm must be"), (dict(dt=0.0), b"nonpositive dt"),
                    (dict(cap=0), b"max_rainsplit"), (dict(cap=1025), b"max_rainsplit"), (dict(nens=65), b"nens must be"),
                    (dict(work=None), b"null pointer"), (dict(fields=None), b"null pointer"), (dict(outs=None), b"null pointer")):
        assert teacher(**kw) != 0 and msg in L.mw_last_error(), kw
    hole = (C.c_void_p * 5)(0x1000, 0x1000, None, 0x1000, 0x1000)
    assert teacher(fields=hole) != 0 and b"null field" in L.mw_last_error()
    mask = C.c_void_p(0x4000)
    assert L.mw_member_sample_mask(4, 16, 3, 1, (C.c_int * 1)(3), f5, o4, 0, 0.5, 0.5, mask, None) != 0 and b"outside [0, 3)" in L.mw_last_error()
    assert L.mw_member_sample_mask(4, 16, 3, 2, (C.c_int * 2)(1, 1), f5, o4, 0, 0.5, 0.5, mask, None) != 0 and b"listed twice" in L.mw_last_error()
    assert L.mw_member_sample_mask(4, 16, 3, 1, (C.c_int * 1)(1), f5, o4, 0, 0.5, 0.5, None, None) != 0 and b"null pointer" in L.mw_last_error()
    assert L.mw_member_gather_samples(4, 16, 3, f5, o4, None, 5, mask, mask, None) != 0 and b"null pointer" in L.mw_last_error()
    assert L.mw_member_gather_samples(4, 16, 3, f5, o4, mask, -1, mask, mask, None) != 0 and b"n must be" in L.mw_last_error()
    if not torch.cuda.is_available():
        assert teacher() != 0 and b"no HIP device" in L.mw_last_error()
        assert L.mw_member_sample_mask(4, 16, 3, 1, (C.c_int * 1)(1), f5, o4, 0, 0.5, 0.5, mask, None) != 0 and b"no HIP device" in L.mw_last_error()
        assert L.mw_member_gather_samples(4, 16, 3, f5, o4, mask, 5, mask, mask, None) != 0 and b"no HIP device" in L.mw_last_error()


# ---- the YAML block -------------------------------------------------------------------------------------------------------------------
def model_list(tmp_path, k):
    from miniweatherml_amd import modules, surrogate_train as st
    W1, b1, W2, b2, si, so = modules.load_surrogate_weights()
    w = st.initial_weights(0, k)
    _, models = st.write_outputs(str(tmp_path / "t"), w[0], si, so, {}, all_weights=w)
    return "surrogate_models:\n" + "".join("  - {%s}\n" % ", ".join('%s: "%s"' % kv for kv in m.items()) for m in models), models


def test_harvest_config_defaults_and_refusals(mw, tmp_path):
    from miniweatherml_amd import driver
    lst, models = model_list(tmp_path, 3)
    names = [m["name"] for m in models]
    p = tmp_path / "in.yaml"
    p.write_text(BASE + lst + "eval_interval: 4\n")
    cfg = driver.load_config(str(p))
    assert driver.harvest_config(cfg) is None
    assert driver.rollout_config(cfg) == (models, 4, True, 5)
    p.write_text(BASE + lst + "eval_interval: 4\nharvest: {}\n")
    cfg = driver.load_config(str(p))
    assert driver.harvest_config(cfg) == {"interval": 4, "samples_per_step": 50, "ratio_active": 0.5, "seed": None, "max_rainsplit": 64,
                                          "members": names}
    assert driver.rollout_config(cfg) == (models, 4, True, 5)                  # the tuple is what it is without the block
    p.write_text(BASE + lst + "harvest:\n")                                    # an empty block: all defaults, interval = eval_interval's default
    assert driver.harvest_config(driver.load_config(str(p)))["interval"] == 1
    p.write_text(BASE + lst + "harvest: {interval: 2, samples_per_step: 200.5, ratio_active: 0.25, seed: 7, max_rainsplit: 8, members: [%s]}\n" % names[1])
    assert driver.harvest_config(driver.load_config(str(p))) == {"interval": 2, "samples_per_step": 200.5, "ratio_active": 0.25, "seed": 7,
                                                                 "max_rainsplit": 8, "members": [names[1]]}
    for bad, msg in (("{every: 2}", "unknown key"), ("{interval: 0}", "interval"), ("{interval: 1.5}", "interval"), ("{interval: true}", "interval"),
                     ("{samples_per_step: 0}", "samples_per_step"), ("{samples_per_step: -3}", "samples_per_step"),
                     ("{samples_per_step: many}", "samples_per_step"), ("{ratio_active: 0}", "ratio_active"), ("{ratio_active: 1}", "ratio_active"),
                     ("{ratio_active: 1.5}", "ratio_active"), ("{max_rainsplit: 0}", "max_rainsplit"), ("{max_rainsplit: 2000}", "max_rainsplit"),
                     ("{seed: -1}", "seed"), ("{seed: 0.5}", "seed"), ("{members: [nobody]}", "no surrogate model"), ("{members: []}", "non-empty"),
                     ("{members: %s}" % names[0], "non-empty list"), ("{members: [%s, %s]}" % (names[0], names[0]), "twice"),
                     ("[1, 2]", "mapping"), ("5", "mapping")):
        p.write_text(BASE + lst + "harvest: %s\n" % bad)
        with pytest.raises(ValueError, match=msg):
            driver.harvest_config(driver.load_config(str(p)))


# ---- the warm start, host side ----------------------------------------------------------------------------------------------------------
def test_init_reads_the_directory_and_refuses_the_other_width(mw, tmp_path):
    from miniweatherml_amd import modules, surrogate_train as st
    rng = np.random.default_rng(4)
    for stencil in (False, True):
        n_in, npar = (9, 144) if stencil else (5, 104)
        w = rng.normal(size=npar).astype(np.float32)
        si = np.sort(rng.normal(size=(n_in, 2)).astype(np.float32).astype(np.float64), axis=1)
        so = np.sort(rng.normal(size=(4, 2)).astype(np.float32).astype(np.float64), axis=1)
        d = tmp_path / ("w%d" % n_in)
        st.write_outputs(str(d), w, si, so, {})
        w0, a, b = st.load_init(str(d), stencil=stencil)
        assert w0.dtype == np.float32 and np.array_equal(w0, w) and np.array_equal(a, si) and np.array_equal(b, so)
        # the tables are the directory's, as the host-side loader reads them
        ref = modules.load_surrogate_weights(*[str(d / f) for f in ("weights.txt", "input_scaling.txt", "output_scaling.txt")])
        assert np.array_equal(a, ref[4]) and np.array_equal(b, ref[5])
        assert np.array_equal(w0, np.concatenate([np.ravel(x) for x in ref[:4]]))
        with pytest.raises(st.SurrogateTrainError, match="parameters"):
            st.load_init(str(d), stencil=not stencil)
    with pytest.raises(st.SurrogateTrainError, match="no file"):
        st.load_init(str(tmp_path / "nothing"))
    (tmp_path / "w5" / "input_scaling.txt").write_text("0 1\n0 1\n0 1\n")       # three rows beside 104 weights
    with pytest.raises(st.SurrogateTrainError, match="scaling rows"):
        st.load_init(str(tmp_path / "w5"))


def test_init_changes_what_data_scaling_refuses():
    """With a warm start the tables are not the data's, so a constant column is no refusal; non-finite values and no samples still are."""
    from miniweatherml_amd import surrogate_train as st
    x = np.random.default_rng(0).normal(size=(20, 5)).astype(np.float32)
    y = np.random.default_rng(1).normal(size=(20, 4)).astype(np.float32)
    x[:, 3] = 0.0
    with pytest.raises(st.SurrogateTrainError, match="constant"):
        st.data_scaling(x, y)
    st.data_scaling(x, y, allow_constant=True)
    x[7, 1] = np.inf
    with pytest.raises(st.SurrogateTrainError, match="non-finite"):
        st.data_scaling(x, y, allow_constant=True)
    with pytest.raises(st.SurrogateTrainError, match="zero samples"):
        st.data_scaling(x[:0], y[:0], allow_constant=True)


def test_init_is_on_the_command_line():
    from miniweatherml_amd import surrogate_train as st
    import inspect
    assert "init" in inspect.signature(st.train_surrogate).parameters and "initial" in inspect.signature(st.Trainer.__init__).parameters
    assert "--init" in inspect.getsource(st.main)
