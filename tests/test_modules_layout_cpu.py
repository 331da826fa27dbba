"""The host-side modules' layout without a GPU: `modules` re-exports, under the names it has always had, what the topical modules define;
each of them imports on its own; MW_OPTIONS still fills the one option table; and the pure-numpy helpers that the reports share."""
import ast
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the public names of modules.py before it was split, in its order, each with the module that defines it now
HOMES = {
    "dycore": ["DEFAULT_OPTIONS", "PATH_LOG", "Dynamics_Euler_Stratified_WenoFV", "perturb_temperature"],
    "microphysics": ["Microphysics_Kessler", "Microphysics_Kessler_Surrogate"],
    "mlp": ["load_h5_weights", "load_surrogate_weights", "mlp_forward", "mlp_stencil_forward", "stencil_features", "ponni_forward",
            "load_surrogate_bank", "_PonniLayer"],
    "surrogate_eval": ["EVAL_FIELDS", "EVAL_CLASSES", "SurrogateBank", "json_safe", "surrogate_scores", "SurrogateEvaluator", "committee_score",
                       "range_error_correlation", "CommitteeEvaluator", "_sums_to_float"],
    "rollout": ["ROLLOUT_FIELDS", "ROLLOUT_STATS", "ROLLOUT_WATER", "ROLLOUT_IN5", "rollout_member_names", "Microphysics_Rollout",
                "kessler_members_teacher", "RolloutHarvester", "member_divergence", "rollout_report", "RolloutScorer"],
    "exchange": ["use_rccl_allreduce", "install_exchange", "use_rccl_exchange", "use_rccl_self_exchange", "use_torch_distributed_exchange"],
    "column": ["set_column_strict", "sponge_layer", "ColumnNudger"],
    "ncio": ["dycore_output"],
    "city": ["Horizontal_Sponge", "Time_Averager"],
    "sampling": ["StatisticsGatherer", "DataGenerator"],
    "experiments": ["make_supercell", "make_simple_city", "simple_city_step", "supercell_step"],
    "_ffi": ["_ptr", "_stream_ptr", "_field_ptr_array"],
    "capi": ["MWError", "check"],
    "coupler": ["Coupler", "endrun"],
}
NEW_MODULES = [m for m in HOMES if m not in ("capi", "coupler")]


def child(code, **env):
    return subprocess.Popen([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                            text=True)


def test_every_name_is_on_the_facade_and_is_its_home_object():
    import importlib
    from miniweatherml_amd import capi, modules, ncio
    public = [n for names in HOMES.values() for n in names if not n.startswith("_") and n not in ("MWError", "check", "Coupler", "endrun")]
    assert len(public) == len(set(public)) == 50
    for home, names in HOMES.items():
        mod = importlib.import_module("miniweatherml_amd." + home)
        for n in names:
            assert getattr(modules, n) is getattr(mod, n), (home, n)
    assert modules.capi is capi and modules._NcFile is ncio.NcFile
    assert isinstance(modules.DEFAULT_OPTIONS, dict) and isinstance(modules.PATH_LOG, list)
    assert modules.Dynamics_Euler_Stratified_WenoFV.output.__module__ == "miniweatherml_amd.dycore"       # a method of the class, no late patch


def test_the_facade_defines_nothing():
    tree = ast.parse(open(os.path.join(ROOT, "miniweatherml_amd", "modules.py")).read())
    assert isinstance(tree.body[0], ast.Expr) and isinstance(tree.body[0].value, ast.Constant) and isinstance(tree.body[0].value.value, str)
    for node in tree.body[1:]:
        all_list = isinstance(node, ast.Assign) and [getattr(t, "id", None) for t in node.targets] == ["__all__"]
        assert isinstance(node, (ast.Import, ast.ImportFrom)) or all_list, ast.dump(node)


def test_each_module_imports_alone():
    names = NEW_MODULES + ["modules"]
    for first in range(0, len(names), 4):                                           # four interpreters at a time
        procs = {m: child("import miniweatherml_amd.%s" % m) for m in names[first:first + 4]}
        for m, p in procs.items():
            _, err = p.communicate(timeout=300)
            assert p.returncode == 0, (m, err[-2000:])


def test_mw_options_fills_the_one_table():
    p = child("from miniweatherml_amd import dycore, modules\n"
              "print(modules.DEFAULT_OPTIONS == {'pipe': 0, 'chunk_z': 7}, modules.DEFAULT_OPTIONS is dycore.DEFAULT_OPTIONS)",
              MW_OPTIONS="pipe=0,chunk_z=7")
    out, err = p.communicate(timeout=300)
    assert p.returncode == 0 and out.split() == ["True", "True"], (out, err[-2000:])


def test_finite_or_none():
    from miniweatherml_amd.surrogate_eval import finite_or_none
    fine = {"bias": -1.0, "mae": 1.0, "rmse": 2.0, "max_abs": 3.0, "rmse_over_persistence": 0.5}
    assert finite_or_none(dict(fine)) == fine
    no_ratio = dict(fine, rmse_over_persistence=None)
    assert finite_or_none(dict(no_ratio)) == no_ratio
    got = finite_or_none(dict(fine, mae=float("nan"), max_abs=float("inf")))
    assert got == dict(fine, mae=None, max_abs=None, finite=False) and list(got)[-1] == "finite"
    assert finite_or_none(dict(no_ratio, bias=float("-inf"))) == dict(no_ratio, bias=None, finite=False)


def test_exact_units_split_and_back():
    from miniweatherml_amd.surrogate_eval import _exact_units_array, _sums_to_float
    x = np.array([0.0, 5e-324, -1.5, np.inf, np.nan])
    units, nonfinite = _exact_units_array(x)
    assert units.dtype == object and list(units) == [0, 1, -3 * 2 ** 1073, 0, 0]
    assert list(nonfinite[:3]) == [0.0, 0.0, 0.0] and nonfinite[3] == np.inf and np.isnan(nonfinite[4])
    back = _sums_to_float(units, nonfinite)
    assert np.array_equal(back[:3].view(np.uint64), x[:3].view(np.uint64)) and back[3] == np.inf and np.isnan(back[4])
    assert list((units + units)[:3]) == [0, 2, -3 * 2 ** 1074]                        # integers: addition is exact


def test_skill_cell():
    from miniweatherml_amd.surrogate_eval import skill_cell
    assert skill_cell(None, None) == " " * 25 + "-"
    assert skill_cell(1.0, None) == " " * 10 + "1.000000e+00 (-)"
    assert skill_cell(1.0, 0.5) == " " * 8 + "1.000000e+00 (0.5)"
