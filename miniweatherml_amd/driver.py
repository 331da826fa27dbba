"""YAML-driven drivers: the reference's experiment mains over the MI355X-native modules.

    python -m miniweatherml_amd.driver <experiment> <input.yaml> [--max-steps N] [--device cuda:0]
    torchrun --nproc-per-node N -m miniweatherml_amd.driver <experiment> <input.yaml>          # one rank per GPU

experiment            reference main                                                    loop body
supercell_example     experiments/supercell_example/driver.cpp:12-89                    dycore, Kessler, sponge_layer, ColumnNudger
community_benchmark   experiments/community_benchmark/driver.cpp:12-92                  the same, timed as "simulation_loop" (:66,82)
simple_city           experiments/simple_city/driver.cpp:9-88                           horiz. sponge, dycore, sponge_layer(dt,1), averager
inference_ponni       experiments/supercell_kessler_surrogate/inference_ponni.cpp        dycore, NN + Kessler, sponge, nudger
gather_statistics     experiments/supercell_kessler_surrogate/gather_statistics.cpp      dycore, Kessler (+ active-cell ratio), sponge, nudger
generate_micro_data   experiments/supercell_kessler_surrogate/generate_micro_data.cpp    dycore, Kessler (+ training samples), sponge, nudger
evaluate_surrogates   (none: gather_statistics' loop)                                    dycore, Kessler (+ scores of candidate networks), sponge, nudger
rollout_surrogates    (none: the same loop, one ensemble member per candidate)           dycore, Kessler | network | nothing per member, sponge, nudger

The YAML keys are the reference's (sim_time, nens, nx_glob, ny_glob, nz, xlen, ylen, zlen, dt_phys, out_prefix, init_data,
out_freq, enable_gravity, file_per_process; keras_weights_h5 / nn_input_scaling / nn_output_scaling for the surrogate).  The
Keras HDF5 file named by `keras_weights_h5` is read by the library's own reader (mw_h5.cpp = ponni::load_h5_weights); a text export
(`keras_weights_txt`, tools/export_mlp_weights.sh) is accepted too; without either, the reference's shipped weight file
(miniweatherml_amd/data/) is used.

evaluate_surrogates scores the networks of a YAML list against the Kessler scheme that runs the simulation (surrogate_eval.SurrogateEvaluator):
    surrogate_models:
      - {name: seed0, keras_weights_txt: out/weights_0.txt, nn_input_scaling: out/input_scaling.txt, nn_output_scaling: out/output_scaling.txt}
      - ...                                   # (keras_weights_h5 instead of keras_weights_txt for a Keras file; both widths may be mixed)
    eval_interval: 1                          # evaluate every n-th step (default 1)
and writes surrogate_evaluation.json (the report and the per-call history) into the working directory.  One rank only.

rollout_surrogates reads the same list and runs every network ONLINE, as an ensemble member of its own beside Kessler (member 0; members
1 .. K the list's models in its order, rollout.Microphysics_Rollout): each member's output is fed back through the dycore, and every
eval_interval-th step all eight coupler fields of every member are scored against the Kessler member (rollout.RolloutScorer).
    persistence_member: true                  # a last member without microphysics, the skill's denominator (default true)
nens is derived from the list (1 + K, + 1 with the persistence member); a `nens:` key that disagrees is an error.  Writes
surrogate_rollout.json.  One rank only.
    harvest: {interval: 10, samples_per_step: 50, ratio_active: 0.5, seed: 1, max_rainsplit: 64, members: [seed0]}
adds data aggregation to the rollout (rollout.RolloutHarvester): every interval-th step (default eval_interval) Kessler is asked what it
would have done to each listed model member's OWN state (default: all models), and samples of that go to rollout_samples_<name>.nc in the
working directory -- DataGenerator's format, so `surrogate_train --init DIR` continues a model on the old and the new files together.
    surrogate_committees:
      - {name: mean3, members: [seed0, seed1, seed2]}      # 1 .. 16 models of the list above, all of one width
makes committees of the listed models (committee_config; surrogate_eval.SurrogateBank.committee_apply: the mean of the members' outputs in the
listed order, and their range).  rollout_surrogates rolls each committee out as one more member after the models (nens counts them; a
committee cannot be harvested), evaluate_surrogates scores each one (surrogate_eval.CommitteeEvaluator; `committees` in the JSON and the table),
and inference_ponni runs the committee instead of one network when the YAML names exactly one and no keras_weights_* key.
      - {name: guarded3, members: [seed0, seed1, seed2], guard: {precip_liquid: 1.0e-5, temp: 0.5, max_rainsplit: 64}}
is a GUARDED committee: where the range of its models exceeds a threshold at some level of a column (field units; a
field left out never flags by size; a non-finite mean always flags), Kessler takes that column in that step, with rain sub-cycles from
the flagged columns alone (more than max_rainsplit, default 64: the mean stays).  surrogate_rollout.json gets a `guard` block per
guarded committee: the thresholds, `columns`, `flagged_total`, and `flagged` / `rainsplit` at every scoring step.  inference_ponni runs
the guarded step when its one committee has a guard; evaluate_surrogates, which scores the mean, refuses an entry with a guard.
    surface_rain: {thresholds_mm_h: [0.1, 1, 5, 10, 25], thresholds_mm: [0.1, 1, 5, 10, 25], map: true}
makes rollout_surrogates score rain at the ground: every member's precl becomes what its microphysics step removed from
its column's water (the Kessler member keeps Kessler's own), and surrogate_rollout.json gets a `surface_rain` block -- the thresholds and,
per scoring step and member, the statistics of the rate (mm/h) and of the accumulated rain (mm) against the Kessler member with a
contingency table per threshold (rollout.RainScorer).  `map: true` writes surrogate_rollout_rain.npy, float64 (nens, ny, nx), mm, at
the end.  `surface_rain: true` means these defaults; false or absent: off, and the document is what it is without the key.
    training_domain: true                     # or {margin: 0.05, fields: [temp, water_vapor]}
makes rollout_surrogates report, at every scoring step and for every network-stepped member, how much of the member's state lies outside
the box its model was trained in: the rows of a model's input scaling table are the minimum and maximum of each input
over its training samples, a committee's box is the intersection of its models', `margin` widens it by that fraction of its width and
`fields` restricts it.  Every entry of `models` and `committees` in surrogate_rollout.json gets a `domain` block: margin, fields, box,
cells, columns, first_outside_step and, per scoring step, outside_columns and the cells below / above / nan per field.  The report
only reads the state.  Inside a committee's guard,
      - {name: boxed, members: [tend0], guard: {domain: {margin: 0.0}}}
`domain:` (true or the same mapping) hands Kessler every column of the member that holds a cell outside the committee's box, beside the
columns the thresholds flag (a guard may hold only `domain`: a committee of ONE model then has a guard that acts).  Its guard block
gains `domain` (margin, fields, box) and outside_columns per scoring step; flagged stays the union.  rollout_surrogates and
inference_ponni honour it.
    harvest: {interval: 10, samples_per_step: 100, seed: 1, outside: {share: 0.5, margin: 0.0, fields: [temp, water_vapor]}}
`outside:` (true: share 0.5, margin 0, all five fields) makes the harvester ask `share` of samples_per_step of the cells the member has
carried OUTSIDE its model's training box -- the only cells whose label the model has never seen.  Their number is
counted in the call itself, so the rate follows the member; the rest of samples_per_step is drawn from the active and inactive cells as
before.  The sample files keep their format; the `harvest` block of surrogate_rollout.json gains `outside` (share, margin, fields, the
members' boxes), `taken` and `eligible` (per member: outside / active / inactive).
      - {name: tend1, keras_weights_txt: ft/weights.txt, nn_input_scaling: ft/input_scaling.txt, nn_output_scaling: ft/output_scaling.txt,
         nn_training_domain: ft/training_domain.txt}
`nn_training_domain` (optional) names the table `surrogate_train --init DIR` writes beside a continued model: per input the minimum and
maximum over ALL samples the model and the models it continues were trained on, where input_scaling.txt stays the first model's.
training_domain, a guard's domain and harvest.outside then read the model's box from it, not from the scaling rows.
    eval_domain: true                         # or {margin: 0.05, fields: [temp, water_vapor], box_of: seed0}
makes evaluate_surrogates split every model's one-step errors by whether the cell lies inside or outside the model's training box
(surrogate_eval.DomainSplitEvaluator): how much of the error comes from extrapolation.  The boxes are training_domain's
(`margin`, `fields`, nn_training_domain honoured); `box_of` names one entry of surrogate_models whose box then serves every model, so that
a continued model and its parent are scored on the same partition.  surrogate_evaluation.json gains a `domain` block (margin, fields,
box_of, group, per model its box and report, and the per-call history) and a second table is printed; false or absent: no further call
is made and the document is what it is without the key.
    water_fixer: true                         # or {members: [tend0, mean3], tolerance: 0.0}
makes the listed members of rollout_surrogates (default: every model and committee member; never kessler or persistence) give back the
water their model made: a column that holds more water after the microphysics step than before it, by more than
tolerance times what it held, has its three water fields scaled back to what it held.  temp is not touched: a mass fixer, no latent
heat.  The fixed members become budget members (their precl is the water budget of the state left behind) and rain_total exists with
or without surface_rain.  surrogate_rollout.json gets a `water_fixer` block: tolerance, members, columns, per scoring step and member
columns_fixed, columns_skipped and water_removed_kg_m2 {mean over the columns, max}, and the totals over the scoring steps.  Listing
one set of weights under two names and fixing one of them shows the fixer's effect in one run.  inference_ponni reads the key (without
`members`) and then runs its network online with the fixer on every column.  false or absent: the document and the run are what they are
without the key.
    heat_closure: true                        # or {members: [kessler, tend0], closed: [tend0], tolerance: 0.0}
makes rollout_surrogates hold its members to Kessler's latent-heat identity: in a Kessler step a cell's temp changes by
(lv / cp_d) * (its loss of water vapour) / density_dry and by nothing else.  `members` (default: every member but persistence) are
diagnosed: their residual temp - (that value) is measured per cell.  `closed` (default: every model and committee member; never kessler
or persistence; a subset of members) have their temp replaced by the diagnosed value where |residual| > tolerance (K), after the networks
and before the water fixer.  surrogate_rollout.json gets a `heat_closure` block: lv, cp_d, tolerance, members, closed, cells, per scoring
step and member cells_closed, cells_skipped, residual_K {bias, mae, rmse, max} (before closing) and heating_W_m2 {mean, max} (the
spurious heating of a column), and the totals over the scoring steps.  The kessler row is the report's sanity line: a few ulp of temp.
inference_ponni reads the key (without the lists) and then runs its network online with the closure on every cell.  false or absent: the
document and the run are what they are without the key.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import yaml

from . import city, column, microphysics, mlp, rollout, sampling, surrogate_eval
from .coupler import Coupler
from .dycore import Dynamics_Euler_Stratified_WenoFV, perturb_temperature
from .experiments import simple_city_step

EXPERIMENTS = ("supercell_example", "community_benchmark", "simple_city", "inference_ponni", "gather_statistics", "generate_micro_data",
               "evaluate_surrogates", "rollout_surrogates")


def load_config(path):
    """The `config["key"].as<T>()` reads of the reference mains, with their defaults (driver.cpp:22-38)."""
    with open(path) as f:
        cfg = yaml.safe_load(f)
    if not isinstance(cfg, dict):
        raise ValueError("ERROR: Invalid YAML input file")                      # driver.cpp:25
    out = {}
    for key, typ in (("sim_time", float), ("nx_glob", int), ("ny_glob", int), ("nz", int), ("xlen", float), ("ylen", float),
                     ("zlen", float), ("dt_phys", float), ("out_prefix", str), ("init_data", str), ("out_freq", float)):
        if key not in cfg:
            raise KeyError("ERROR: missing key '%s' in the YAML input file" % key)
        out[key] = typ(cfg[key])
    out["nens"] = int(cfg.get("nens", 1))
    out["_nens_given"] = "nens" in cfg                                         # (rollout_surrogates derives nens: rollout_config)
    out["enable_gravity"] = bool(cfg.get("enable_gravity", True))
    out["file_per_process"] = bool(cfg.get("file_per_process", False))
    for key in ("keras_weights_h5", "keras_weights_txt", "nn_input_scaling", "nn_output_scaling"):
        if key in cfg:
            out[key] = str(cfg[key])
    out["_dir"] = os.path.dirname(os.path.abspath(path))
    for key in ("surrogate_models", "eval_interval", "persistence_member", "harvest", "surrogate_committees", "surface_rain", "training_domain", "eval_domain", "water_fixer", "heat_closure"):    # read by surrogate_config / rollout_config / harvest_config / committee_config / surface_rain_config / training_domain_config / eval_domain_key / water_fixer_config / heat_closure_config alone
        if key in cfg:
            out[key] = cfg[key]
    return out


def surrogate_config(cfg):
    """(models, eval_interval) of a loaded configuration for evaluate_surrogates: the checked `surrogate_models` list with its files
    resolved.  Only that experiment calls it: a list left in the YAML of another experiment is not looked at."""
    if "surrogate_models" not in cfg:
        raise KeyError("ERROR: missing key 'surrogate_models' in the YAML input file")
    interval = int(cfg.get("eval_interval", 1))
    if interval < 1:
        raise ValueError("ERROR: eval_interval must be >= 1")
    return _surrogate_models(cfg["surrogate_models"], cfg["_dir"]), interval


COMMITTEE_KEYS = ("name", "members", "guard")


def _model_width(m):
    """5 (single cell) or 9 (stencil): the rows of a checked surrogate model's input scaling table (load_surrogate_weights' rule)."""
    with open(m["nn_input_scaling"]) as f:
        return sum(1 for ln in f if ln.split("#")[0].strip())


def committee_config(cfg):
    """The checked `surrogate_committees:` list of a loaded configuration, [] without the key: entries {name, members: [model names]} --
    1 .. 16 distinct models of `surrogate_models`, all of one width; committee names unique and no model's name, 'kessler' or
    'persistence'.  An entry may carry `guard:` (surrogate_eval.guard_config: thresholds per field and max_rainsplit), which makes it a
    guarded committee; a guarded and an unguarded committee of the same models may stand side by side under two names.  Returns
    [{"name", "members"}] in the YAML's order, with "guard" (the checked mapping) where the entry has one."""
    from . import capi
    from .surrogate_eval import guard_config
    if "surrogate_committees" not in cfg:
        return []
    models, _ = surrogate_config(cfg)
    names = [m["name"] for m in models]
    entries = cfg["surrogate_committees"]
    if not isinstance(entries, list) or not entries:
        raise ValueError("ERROR: surrogate_committees must be a non-empty list")
    out = []
    for e in entries:
        if not isinstance(e, dict) or "name" not in e or "members" not in e:
            raise KeyError("ERROR: every entry of surrogate_committees needs a 'name' and 'members'")
        unknown = sorted(set(e) - set(COMMITTEE_KEYS))
        if unknown:
            raise ValueError("ERROR: unknown key(s) %s in a surrogate_committees entry (known: %s)" % (", ".join(map(repr, unknown)), ", ".join(COMMITTEE_KEYS)))
        cname = str(e["name"])
        if not isinstance(e["members"], list) or not e["members"]:
            raise ValueError("ERROR: committee %r: members must be a non-empty list of model names" % cname)
        members = [str(n) for n in e["members"]]
        for n in members:
            if n not in names:
                raise ValueError("ERROR: committee %r names %r, which is no surrogate model (%s)" % (cname, n, ", ".join(names)))
        if len(set(members)) != len(members):
            raise ValueError("ERROR: committee %r names a model twice" % cname)
        if len(members) > capi.MW_COMMITTEE_MAX_MODELS:
            raise ValueError("ERROR: committee %r has %d models, a committee holds at most %d" % (cname, len(members), capi.MW_COMMITTEE_MAX_MODELS))
        if len({_model_width(models[names.index(n)]) for n in members}) != 1:
            raise ValueError("ERROR: committee %r mixes single-cell and stencil models: a committee has one width" % cname)
        if cname in names or cname in ("kessler", "persistence"):
            raise ValueError("ERROR: committee name %r collides with a surrogate model, 'kessler' or 'persistence'" % cname)
        out.append({"name": cname, "members": members})
        if "guard" in e:
            out[-1]["guard"] = guard_config(e["guard"], "the guard of committee %r" % cname)
    if len({c["name"] for c in out}) != len(out):
        raise ValueError("ERROR: the names of surrogate_committees must be unique")
    return out


def evaluation_committees(cfg):
    """committee_config for evaluate_surrogates, which scores a committee's mean and range against the microphysics in charge and has no
    guarded step to score: an entry with a `guard:` is refused, not scored without it under a name that claims one."""
    committees = committee_config(cfg)
    for c in committees:
        if "guard" in c:
            raise ValueError("ERROR: evaluate_surrogates scores a committee's mean and does not apply a guard: committee %r has one "
                             "(rollout_surrogates and inference_ponni run guarded committees)" % c["name"])
    return committees


def rollout_config(cfg):
    """(models, eval_interval, persistence, nens) of a loaded configuration for rollout_surrogates: surrogate_config's list and interval,
    `persistence_member` (default true) and the member count they imply -- Kessler, one member per model, one per committee of
    `surrogate_committees` (committee_config), persistence.  A `nens` in the YAML that disagrees is an error, and so are more members than
    the dycore steps in one call."""
    from . import capi
    models, interval = surrogate_config(cfg)
    persistence = cfg.get("persistence_member", True)
    if not isinstance(persistence, bool):
        raise ValueError("ERROR: persistence_member must be true or false")
    ncom = len(committee_config(cfg))
    com = (", %d surrogate_committees" % ncom) if ncom else ""
    nens = 1 + len(models) + ncom + (1 if persistence else 0)
    if nens > capi.MW_ROLLOUT_MAX_MEMBERS:
        raise ValueError("ERROR: %d surrogate_models%s%s beside Kessler are %d ensemble members, the dycore steps at most %d"
                         % (len(models), com, " and the persistence member" if persistence else "", nens, capi.MW_ROLLOUT_MAX_MEMBERS))
    if cfg.get("_nens_given") and int(cfg["nens"]) != nens:
        raise ValueError("ERROR: nens = %d in the YAML input file, but %d surrogate_models%s%s beside Kessler are %d members (leave nens out)"
                         % (cfg["nens"], len(models), com, " and the persistence member" if persistence else "", nens))
    if {"kessler", "persistence"} & {m["name"] for m in models}:
        raise ValueError("ERROR: 'kessler' and 'persistence' name members of their own: no surrogate model may be called so")
    return models, interval, persistence, nens


HARVEST_KEYS = ("interval", "samples_per_step", "ratio_active", "seed", "max_rainsplit", "members", "outside")
HARVEST_OUTSIDE_KEYS = ("share", "margin", "fields")


def harvest_outside_config(o):
    """The checked `harvest.outside:` key: true -- share 0.5, margin 0, all five input fields -- or a mapping with
    `share` (a number in (0, 1], not a bool: the part of samples_per_step asked of the cells outside the member's training box) and
    domain_config's `margin` and `fields`.  Returns {"share": float, "margin": float, "fields": [names]}."""
    from .surrogate_eval import domain_config
    o = {} if o is True else o
    if not isinstance(o, dict):
        raise ValueError("ERROR: harvest.outside must be true or a mapping")
    unknown = sorted(set(o) - set(HARVEST_OUTSIDE_KEYS), key=str)
    if unknown:
        raise ValueError("ERROR: unknown key(s) %s in harvest.outside (known: %s)" % (", ".join(map(repr, unknown)), ", ".join(HARVEST_OUTSIDE_KEYS)))
    share = o.get("share", 0.5)
    if isinstance(share, bool) or not isinstance(share, (int, float)) or not 0.0 < share <= 1.0:
        raise ValueError("ERROR: harvest.outside.share must be a number in (0, 1], got %r" % (share,))
    return dict(share=float(share), **domain_config({k: v for k, v in o.items() if k != "share"}, "harvest.outside"))


def harvest_config(cfg):
    """The checked `harvest:` block of a loaded configuration for rollout_surrogates, or None without one: interval (default
    eval_interval), samples_per_step (50), ratio_active (0.5), seed (None: the clock), max_rainsplit (64), members (model names; default all
    models of the list), and -- only when the YAML has the key -- outside (harvest_outside_config).  Only that experiment calls it, after
    rollout_config's checks."""
    if "harvest" not in cfg:
        return None
    h = cfg["harvest"]
    h = {} if h is None else h
    if not isinstance(h, dict):
        raise ValueError("ERROR: harvest must be a mapping")
    unknown = sorted(set(h) - set(HARVEST_KEYS))
    if unknown:
        raise ValueError("ERROR: unknown key(s) %s in harvest (known: %s)" % (", ".join(map(repr, unknown)), ", ".join(HARVEST_KEYS)))
    models, eval_interval = surrogate_config(cfg)
    names = [m["name"] for m in models]
    out = {"interval": h.get("interval", eval_interval), "samples_per_step": h.get("samples_per_step", 50),
           "ratio_active": h.get("ratio_active", 0.5), "seed": h.get("seed"), "max_rainsplit": h.get("max_rainsplit", 64),
           "members": h.get("members", names)}
    for key in ("interval", "max_rainsplit"):
        if isinstance(out[key], bool) or not isinstance(out[key], int) or out[key] < 1:
            raise ValueError("ERROR: harvest.%s must be an integer >= 1" % key)
    if out["max_rainsplit"] > 1024:
        raise ValueError("ERROR: harvest.max_rainsplit must be at most 1024")
    if isinstance(out["samples_per_step"], bool) or not isinstance(out["samples_per_step"], (int, float)) or not out["samples_per_step"] > 0:
        raise ValueError("ERROR: harvest.samples_per_step must be a number > 0")
    if isinstance(out["ratio_active"], bool) or not isinstance(out["ratio_active"], (int, float)) or not 0.0 < out["ratio_active"] < 1.0:
        raise ValueError("ERROR: harvest.ratio_active must be in (0, 1)")
    if out["seed"] is not None and (isinstance(out["seed"], bool) or not isinstance(out["seed"], int) or out["seed"] < 0):
        raise ValueError("ERROR: harvest.seed must be an integer >= 0")
    if not isinstance(out["members"], list) or not out["members"]:
        raise ValueError("ERROR: harvest.members must be a non-empty list of model names")
    out["members"] = [str(n) for n in out["members"]]
    committee_names = [c["name"] for c in committee_config(cfg)]
    for n in out["members"]:
        if n in committee_names:
            raise ValueError("ERROR: harvest.members names %r, which is a committee: only single models are harvested (%s)" % (n, ", ".join(names)))
        if n not in names:
            raise ValueError("ERROR: harvest.members names %r, which is no surrogate model (%s)" % (n, ", ".join(names)))
    if len(set(out["members"])) != len(out["members"]):
        raise ValueError("ERROR: harvest.members names a model twice")
    if "outside" in h and h["outside"] is not False:                        # (false: off, as without the key)
        out["outside"] = harvest_outside_config(h["outside"])
    return out


def harvest_block(harvest, harvester):
    """The `harvest` block of surrogate_rollout.json: the checked configuration, the harvester's files, samples, skipped and calls, and
    -- only for a harvester with `outside` -- outside (the configuration with the members' boxes), taken and eligible per member and
    class (rollout.harvest_outside_report).  Pure Python."""
    from .rollout import harvest_outside_report
    block = dict(harvest, files=dict(harvester.files), samples=dict(harvester.samples), skipped=dict(harvester.skipped), calls=harvester.calls)
    if harvester.outside is not None:
        block.update(harvest_outside_report(harvester.outside, harvester.member_names, harvester.boxes, harvester.taken, harvester.eligible))
    return block


SURFACE_RAIN_KEYS = ("thresholds_mm_h", "thresholds_mm", "map")


def surface_rain_config(cfg):
    """The checked `surface_rain:` block of a loaded configuration for rollout_surrogates, or None when it is absent or false:
    thresholds_mm_h (the events of the rain rate) and thresholds_mm (of the accumulated rain), each 1 .. 8 positive numbers, strictly
    ascending (default 0.1, 1, 5, 10, 25), and map (default true: write surrogate_rollout_rain.npy).  `surface_rain: true` means the
    defaults."""
    from .rollout import RAIN_DEFAULT_THRESHOLDS, rain_thresholds
    b = cfg.get("surface_rain", False)
    if b is False or b is None:
        return None
    b = {} if b is True else b
    if not isinstance(b, dict):
        raise ValueError("ERROR: surface_rain must be true, false or a mapping")
    unknown = sorted(set(b) - set(SURFACE_RAIN_KEYS))
    if unknown:
        raise ValueError("ERROR: unknown key(s) %s in surface_rain (known: %s)" % (", ".join(map(repr, unknown)), ", ".join(SURFACE_RAIN_KEYS)))
    out = {key: rain_thresholds(b.get(key, list(RAIN_DEFAULT_THRESHOLDS)), "surface_rain." + key) for key in SURFACE_RAIN_KEYS[:2]}
    out["map"] = b.get("map", True)
    if not isinstance(out["map"], bool):
        raise ValueError("ERROR: surface_rain.map must be true or false")
    return out


WATER_FIXER_KEYS = ("members", "tolerance")


def water_fixer_config(cfg, member_names=None):
    """The checked `water_fixer:` key of a loaded configuration for rollout_surrogates (and, without `members`, inference_ponni), or None
    when it is absent or false: true (every network-stepped member, tolerance 0) or {members: [names], tolerance: t}.  members: a non-empty
    list of distinct names, never kessler or persistence -- and, when member_names (the names a network steps) is given, each one of them;
    absent: all of them (None in the result).  tolerance: a finite number >= 0 (default 0): a column is fixed when its water grew by more
    than tolerance times what it held."""
    b = cfg.get("water_fixer", False)
    if b is False or b is None:
        return None
    b = {} if b is True else b
    if not isinstance(b, dict):
        raise ValueError("ERROR: water_fixer must be true, false or a mapping")
    unknown = sorted(set(b) - set(WATER_FIXER_KEYS), key=str)
    if unknown:
        raise ValueError("ERROR: unknown key(s) %s in water_fixer (known: %s)" % (", ".join(map(repr, unknown)), ", ".join(WATER_FIXER_KEYS)))
    out = {"members": None, "tolerance": microphysics.water_fix_tolerance(b.get("tolerance", 0.0), "water_fixer.tolerance")}
    if b.get("members") is not None:
        names = b["members"]
        if not isinstance(names, list) or not names or not all(isinstance(n, str) for n in names) or len(set(names)) != len(names):
            raise ValueError("ERROR: water_fixer.members must be a non-empty list of distinct member names")
        for n in names:
            if n in ("kessler", "persistence"):
                raise ValueError("ERROR: water_fixer.members names %r: only a member that a network steps can be fixed" % n)
            if member_names is not None and n not in member_names:
                raise ValueError("ERROR: water_fixer.members names %r, which is no model or committee of this run (%s)"
                                 % (n, ", ".join(member_names)))
        out["members"] = list(names)
    return out


HEAT_CLOSURE_KEYS = ("members", "closed", "tolerance")


def heat_closure_config(cfg, member_names=None, stepped_names=None):
    """The checked `heat_closure:` key of a loaded configuration for rollout_surrogates (and, without the lists, inference_ponni), or None
    when it is absent or false: true (every member but persistence diagnosed, every network-stepped member closed, tolerance 0) or
    {members: [names], closed: [names], tolerance: t}.  members: a non-empty list of distinct names, never persistence -- and, when
    member_names (the rollout's diagnosable members) is given, each one of them; absent: all of them (None in the result).  closed: a list
    (it may be empty: diagnose only) of distinct names, never kessler or persistence, each in `members` when that is given -- and, when
    stepped_names (the names a network steps) is given, each one of them; absent: every network-stepped member among `members` (None).
    tolerance: a finite number >= 0 (default 0), K: a cell is closed when |residual| exceeds it."""
    b = cfg.get("heat_closure", False)
    if b is False or b is None:
        return None
    b = {} if b is True else b
    if not isinstance(b, dict):
        raise ValueError("ERROR: heat_closure must be true, false or a mapping")
    unknown = sorted(set(b) - set(HEAT_CLOSURE_KEYS), key=str)
    if unknown:
        raise ValueError("ERROR: unknown key(s) %s in heat_closure (known: %s)" % (", ".join(map(repr, unknown)), ", ".join(HEAT_CLOSURE_KEYS)))
    out = {"members": None, "closed": None, "tolerance": microphysics.water_fix_tolerance(b.get("tolerance", 0.0), "heat_closure.tolerance")}
    if b.get("members") is not None:
        names = b["members"]
        if not isinstance(names, list) or not names or not all(isinstance(n, str) for n in names) or len(set(names)) != len(names):
            raise ValueError("ERROR: heat_closure.members must be a non-empty list of distinct member names")
        for n in names:
            if n == "persistence":
                raise ValueError("ERROR: heat_closure.members names 'persistence': a member that nothing steps has no residual")
            if member_names is not None and n not in member_names:
                raise ValueError("ERROR: heat_closure.members names %r, which is no member of this run (%s)" % (n, ", ".join(member_names)))
        out["members"] = list(names)
    if b.get("closed") is not None:
        names = b["closed"]
        if not isinstance(names, list) or not all(isinstance(n, str) for n in names) or len(set(names)) != len(names):
            raise ValueError("ERROR: heat_closure.closed must be a list of distinct member names")
        for n in names:
            if n in ("kessler", "persistence"):
                raise ValueError("ERROR: heat_closure.closed names %r: only a member that a network steps can be closed" % n)
            if stepped_names is not None and n not in stepped_names:
                raise ValueError("ERROR: heat_closure.closed names %r, which is no model or committee of this run (%s)"
                                 % (n, ", ".join(stepped_names)))
            if out["members"] is not None and n not in out["members"]:
                raise ValueError("ERROR: heat_closure.closed names %r, which is not in heat_closure.members" % n)
        out["closed"] = list(names)
    return out


def training_domain_config(cfg):
    """The checked `training_domain:` key of a loaded configuration for rollout_surrogates, or None when it is absent or false: true
    (margin 0, all five input fields) or {margin, fields} (surrogate_eval.domain_config)."""
    from .surrogate_eval import domain_config
    b = cfg.get("training_domain", False)
    if b is False or b is None:
        return None
    return domain_config(b, "training_domain")


def eval_domain_key(cfg, model_names):
    """The checked `eval_domain:` key of a loaded configuration for evaluate_surrogates, or None when it is absent or false
    (surrogate_eval.eval_domain_config: true or {margin, fields, box_of})."""
    from .surrogate_eval import eval_domain_config
    b = cfg.get("eval_domain", False)
    if b is False or b is None:
        return None
    return eval_domain_config(b, model_names)


def _domain_split_evaluator(cfg_domain, evaluator, eval_models):
    """The DomainSplitEvaluator on a SurrogateEvaluator's banks and names: every model's own box (domain_box, its training-domain table
    honoured), or the box of the entry `box_of` names for all of them."""
    weights = mlp.load_surrogate_bank(eval_models)
    tables = mlp.load_training_domains(eval_models, weights)
    names = [m["name"] for m in eval_models]
    def box(k):
        return surrogate_eval.domain_box([weights[k]], cfg_domain["margin"], cfg_domain["fields"], names=[names[k]], tables=[tables[k]])
    if cfg_domain["box_of"] is not None:
        boxes = [box(names.index(cfg_domain["box_of"]))] * len(names)
    else:
        boxes = [box(k) for k in range(len(names))]
    return surrogate_eval.DomainSplitEvaluator(evaluator.banks, names, boxes)


def _surrogate_models(entries, yaml_dir):
    """The `surrogate_models:` list: every entry names a model and its three files (relative paths: from the working directory, as the
    other file keys, else from the YAML file's directory), and optionally `nn_training_domain`, the training_domain.txt of a continued
    model, which every consumer of the model's box then reads in place of the scaling rows."""
    if not isinstance(entries, list) or not entries:
        raise ValueError("ERROR: surrogate_models must be a non-empty list")
    out = []
    for e in entries:
        if not isinstance(e, dict) or "name" not in e:
            raise KeyError("ERROR: every entry of surrogate_models needs a 'name'")
        if ("keras_weights_txt" in e) == ("keras_weights_h5" in e):
            raise KeyError("ERROR: surrogate model %r needs exactly one of keras_weights_txt and keras_weights_h5" % e["name"])
        m = {"name": str(e["name"])}
        for key in ("keras_weights_txt", "keras_weights_h5", "nn_input_scaling", "nn_output_scaling", "nn_training_domain"):
            if key in e:
                p = str(e[key])
                if not os.path.isabs(p):
                    here = os.path.normpath(os.path.join(os.getcwd(), p))
                    p = here if os.path.exists(here) else os.path.normpath(os.path.join(yaml_dir, p))
                if not os.path.exists(p):
                    raise FileNotFoundError("ERROR: surrogate model %r: no file %s" % (e["name"], p))
                m[key] = p
            elif key.startswith("nn_") and key != "nn_training_domain":    # (optional: without it the scaling rows are the domain)
                raise KeyError("ERROR: surrogate model %r needs '%s'" % (e["name"], key))
        out.append(m)
    if len({m["name"] for m in out}) != len(out):
        raise ValueError("ERROR: the names of surrogate_models must be unique")
    return out


def _surrogate_evaluator(entries, device):
    """One bank per width, in the order the widths first appear; the models' names bank after bank."""
    weights = mlp.load_surrogate_bank(entries)
    widths = []
    for w in weights:
        if w[0].shape[0] not in widths:
            widths.append(w[0].shape[0])
    order = [i for n_in in widths for i, w in enumerate(weights) if w[0].shape[0] == n_in]
    banks = [surrogate_eval.SurrogateBank([w for w in weights if w[0].shape[0] == n_in], device) for n_in in widths]
    return surrogate_eval.SurrogateEvaluator(banks, [entries[i]["name"] for i in order]), [entries[i] for i in order]


def _distributed(device):
    """One process per GPU when launched by torchrun; returns (nranks, myrank, device)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1:
        return 1, 0, device
    import torch.distributed as dist
    # dmabuf IPC (the host driver of this pool supports nothing else: without it RCCL between processes fails with
    # "hipIpcGetMemHandle: invalid argument").  The HSA runtime reads it when it initialises -- at the first GPU call, below.
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    rank, local = int(os.environ["RANK"]), int(os.environ.get("LOCAL_RANK", "0"))
    if device.startswith("cuda"):
        device = "cuda:%d" % local
        torch.cuda.set_device(local)
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl" if device.startswith("cuda") else "gloo", rank=rank, world_size=world)
    return world, rank, device


def _coupler(cfg, device, nranks, myrank, yaml_path):
    c = Coupler(device)
    c.set_option("out_prefix", cfg["out_prefix"])
    c.set_option("init_data", cfg["init_data"])
    c.set_option("out_freq", cfg["out_freq"])
    c.set_option("enable_gravity", cfg["enable_gravity"])
    c.set_option("file_per_process", cfg["file_per_process"])
    c.distribute_mpi_and_allocate_coupled_state(cfg["nz"], cfg["ny_glob"], cfg["nx_glob"], cfg["nens"], nranks, myrank)
    c.set_grid(cfg["xlen"], cfg["ylen"], cfg["zlen"])
    c.set_option("standalone_input_file", yaml_path)
    return c


def _exchange(dycore, coupler):
    from . import exchange
    return exchange.install_exchange(dycore, coupler)            # all ranks agree on one transport (RCCL, else torch p2p)


def _time_loop(cfg, dycore, coupler, body, max_steps):
    """while (etime < sim_time) { dtphys = ...; body; etime += dtphys; }   (driver.cpp:66-79)"""
    etime, steps = 0.0, 0
    dtphys = cfg["dt_phys"]
    while etime < cfg["sim_time"] and (max_steps is None or steps < max_steps):
        if cfg["dt_phys"] <= 0.0:
            dtphys = dycore.compute_time_step(coupler)
        if etime + dtphys > cfg["sim_time"]:
            dtphys = cfg["sim_time"] - etime
        body(dtphys, etime)
        etime += dtphys
        steps += 1
    return etime, steps


class Experiment:
    """One experiment of EXPERIMENTS, in four stages that run() calls in this order: configure (the experiment's YAML checks; no device
    is touched yet), setup (the modules, after the coupler and the dycore exist), step (the time loop's body) and finish (reports and
    files, after the loop).  Collaborators are plain attributes, so a test can put recording stubs in their place."""

    timed = False                                                              # True: run() times the loop as info["simulation_loop_s"]

    def configure(self, cfg, nranks):
        pass

    def setup(self, cfg, coupler, dycore, info, device, quiet):
        self.cfg, self.coupler, self.dycore, self.info, self.device, self.quiet = cfg, coupler, dycore, info, device, quiet

    def finish(self, steps, yaml_path):
        pass


def _one_rank(experiment, nranks):
    if nranks > 1:
        raise ValueError("%s runs on one rank (%d given): SurrogateEvaluator.combine is exact, but the reduction over "
                         "ranks is not built yet" % (experiment, nranks))


class SimpleCity(Experiment):
    def setup(self, *args):
        super().setup(*args)
        coupler, dycore = self.coupler, self.dycore
        self.horiz_sponge, self.time_averager = city.Horizontal_Sponge(), city.Time_Averager()
        coupler.add_tracer("water_vapor", "water_vapor", True, True)           # simple_city/driver.cpp:55-56
        coupler.get_data_manager_readwrite().get("water_vapor").zero_()
        dycore.init(coupler)
        _exchange(dycore, coupler)
        self.horiz_sponge.init(coupler, 10, 1.0)
        self.time_averager.init(coupler)

    def step(self, dt, etime):                                                 # :72-75
        simple_city_step(self.coupler, self.dycore, self.horiz_sponge, self.time_averager, dt)

    def finish(self, steps, yaml_path):
        self.time_averager.finalize(self.coupler)                              # :82 -> time_averaged_fields.nc


class Column(Experiment):
    """supercell_example as it stands, and the family of the experiments that run its loop with another microphysics (make_micro), with
    work around the microphysics step (micro_step) or after the nudger (after_step)."""

    def make_micro(self):
        micro = microphysics.Microphysics_Kessler()
        micro.init(self.coupler)                                               # supercell_example/driver.cpp:58
        return micro

    def setup(self, *args):
        super().setup(*args)
        self.nstep = 0                                                         # steps taken so far
        self.nudger = column.ColumnNudger()
        self.micro = self.make_micro()
        self.dycore.init(self.coupler)                                         # :59
        _exchange(self.dycore, self.coupler)
        self.nudger.set_column(self.coupler)                                   # :60
        perturb_temperature(self.coupler)                                      # :61

    def step(self, dt, etime):                                                 # :73-76
        self.dycore.time_step(self.coupler, dt)
        self.micro_step(dt, etime)
        column.sponge_layer(self.coupler, dt)
        self.nudger.nudge_to_column(self.coupler, dt)                          # (eager: a scorer reads the nudged fields)
        self.after_step(dt, etime)
        self.nstep += 1

    def micro_step(self, dt, etime):
        self.micro.time_step(self.coupler, dt)

    def micro_step_keeping_input(self, dt):
        """The microphysics step on the coupler; returns a copy of the state it started from (gather_statistics.cpp:79-80)."""
        inp = Coupler(self.device)
        self.coupler.clone_into(inp)
        self.micro.time_step(self.coupler, dt)
        return inp

    def after_step(self, dt, etime):
        pass


class CommunityBenchmark(Column):
    timed = True                                                               # timer "simulation_loop", community_benchmark/driver.cpp:66,82


class InferencePonni(Column):
    committee = None                                                           # the one committee that runs in place of a single network
    fixer_cfg = None                                                           # the checked `water_fixer` key (without members)
    closure_cfg = None                                                         # the checked `heat_closure` key (without the lists)

    def configure(self, cfg, nranks):
        if "surrogate_committees" in cfg and not ("keras_weights_h5" in cfg or "keras_weights_txt" in cfg):
            committees = committee_config(cfg)
            if len(committees) != 1:
                raise ValueError("ERROR: inference_ponni runs one committee, surrogate_committees lists %d" % len(committees))
            cfg["surrogate_models"], _ = surrogate_config(cfg)
            self.committee = committees[0]
        self.fixer_cfg = water_fixer_config(cfg)
        if self.fixer_cfg is not None and self.fixer_cfg["members"] is not None:
            raise ValueError("ERROR: inference_ponni's water_fixer takes no members: the one network steps every column")
        self.closure_cfg = heat_closure_config(cfg)
        if self.closure_cfg is not None and (self.closure_cfg["members"] is not None or self.closure_cfg["closed"] is not None):
            raise ValueError("ERROR: inference_ponni's heat_closure takes no members and no closed: the one network steps every cell")

    def make_micro(self):
        cfg, coupler, info = self.cfg, self.coupler, self.info
        micro = microphysics.Microphysics_Kessler_Surrogate()
        if self.committee is not None:                                         # the mean of the committee's models is what runs
            by_name = {m["name"]: m for m in cfg["surrogate_models"]}
            entries = [by_name[n] for n in self.committee["members"]]
            bank = mlp.load_surrogate_bank(entries)
            micro.init(coupler, committee=bank, guard=self.committee.get("guard"), domains=mlp.load_training_domains(entries, bank))
        else:
            def rel(p):
                return p if p is None or os.path.isabs(p) else os.path.normpath(os.path.join(os.getcwd(), p))
            h5 = rel(cfg.get("keras_weights_h5"))
            kw = dict(weights_txt=rel(cfg.get("keras_weights_txt")), weights_h5=h5 if h5 and os.path.exists(h5) else None)
            for k_yaml, k_arg in (("nn_input_scaling", "in_scaling_txt"), ("nn_output_scaling", "out_scaling_txt")):
                p = rel(cfg.get(k_yaml))
                kw[k_arg] = p if p and os.path.exists(p) else None             # else: the shipped tables
            micro.init(coupler, **kw)
        # the form travels with the files: the single model's, or every committee model's
        info["surrogate_form"] = micro.form if self.committee is None else micro._committee.forms
        if "tendency" in info["surrogate_form"] and not self.quiet and coupler.is_mainproc():     # (a state model prints what it always did)
            print("inference_ponni: surrogate output form: %s" % info["surrogate_form"], flush=True)
        if self.fixer_cfg is not None:                                         # the fixer acts on the state the network leaves: online
            micro.online, micro.water_fixer = True, {"tolerance": self.fixer_cfg["tolerance"]}
        if self.closure_cfg is not None:                                       # the closure acts on the state the network leaves: online
            micro.online, micro.heat_closure = True, {"tolerance": self.closure_cfg["tolerance"]}
        return micro

    def micro_step(self, dt, etime):
        self.micro.time_step(self.coupler, dt)
        if not self.quiet and self.coupler.is_mainproc():
            d = self.micro.mean_diffs(self.coupler)                            # microphysics_kessler_ponni.h:266-269
            print("Relative diff rho_v: %r\nRelative diff rho_c: %r\nRelative diff rho_r: %r\nRelative diff temp : %r" %
                  (d["rho_v"], d["rho_c"], d["rho_r"], d["temp"]), flush=True)


class GatherStatistics(Column):
    def setup(self, *args):
        super().setup(*args)
        self.stats = sampling.StatisticsGatherer()

    def micro_step(self, dt, etime):
        inp = self.micro_step_keeping_input(dt)
        self.stats.gather_micro_statistics(inp, self.coupler, dt, etime)

    def finish(self, steps, yaml_path):
        self.stats.finalize(self.coupler)
        self.info["ratio_active"] = self.stats.ratio(self.coupler)


class GenerateMicroData(Column):
    def setup(self, *args):
        super().setup(*args)
        self.datagen = sampling.DataGenerator()
        self.datagen.init(self.coupler, os.getcwd())                           # generate_micro_data.cpp:66
        self.info["samples"] = 0

    def micro_step(self, dt, etime):
        inp = self.micro_step_keeping_input(dt)
        self.info["samples"] += self.datagen.generate_samples_stencil(inp, self.coupler, dt, etime)


def evaluation_document(experiment, yaml_path, eval_interval, steps, evaluator, eval_models, eval_calls, rep, committee_evals=(),
                        eval_domain=None, domain_eval=None, drep=None):
    """surrogate_evaluation.json as a dict.  rep, drep: the evaluator's and the DomainSplitEvaluator's reports ({} without a call);
    committee_evals: (committee, its CommitteeEvaluator) pairs; eval_domain: the checked key, None with domain_eval None."""
    doc = {"experiment": experiment, "yaml": os.path.abspath(yaml_path), "eval_interval": eval_interval, "steps": steps,
           "models": [dict(m, bank=ib, n_in=b.n_in, form=b.forms[k]) for ib, b in enumerate(evaluator.banks)
                      for k, m in enumerate(eval_models[sum(x.models for x in evaluator.banks[:ib]):][:b.models])],
           "statistics": ["sum_d", "sum_abs_d", "sum_d2", "max_abs_d"], "fields": list(surrogate_eval.EVAL_FIELDS),
           "classes": list(surrogate_eval.EVAL_CLASSES), "report": rep,
           "history": [dict(c, banks=h) for c, h in zip(eval_calls, evaluator.history)]}
    if committee_evals:
        doc["committees"] = [dict(c, n_in=ce.bank.n_in, statistics=["sum_d", "sum_abs_d", "sum_d2", "max_abs_d", "sum_r", "sum_r2", "sum_r_abs_d"],
                                  report=ce.report() if eval_calls else {}, history=ce.history) for c, ce in committee_evals]
    if domain_eval is not None:
        doc["domain"] = dict(eval_domain, group={str(b.n_in): b.domain_group for b in evaluator.banks},
                             models={n: {"box": surrogate_eval.box_json(domain_eval.boxes[k]), "report": drep.get(n, {})}
                                     for k, n in enumerate(domain_eval.names)},
                             history=[dict(c, banks=h) for c, h in zip(eval_calls, domain_eval.history)])
    return doc


class EvaluateSurrogates(Column):
    def configure(self, cfg, nranks):
        _one_rank("evaluate_surrogates", nranks)
        self.committees = evaluation_committees(cfg)
        cfg["surrogate_models"], cfg["eval_interval"] = surrogate_config(cfg)
        self.eval_domain = eval_domain_key(cfg, [m["name"] for m in cfg["surrogate_models"]])

    def setup(self, *args):
        super().setup(*args)
        self.evaluator, self.eval_models = _surrogate_evaluator(self.cfg["surrogate_models"], self.device)
        self.domain_eval = None
        if self.eval_domain is not None:
            self.domain_eval = _domain_split_evaluator(self.eval_domain, self.evaluator, self.eval_models)
        self.committee_evals = []                                              # (committee, its evaluator on the bank of its width)
        for c in self.committees:
            places = [[m["name"] for m in self.eval_models].index(n) for n in c["members"]]
            first = 0
            for bank in self.evaluator.banks:
                if first <= places[0] < first + bank.models:
                    self.committee_evals.append((c, surrogate_eval.CommitteeEvaluator(bank, [i - first for i in places])))
                first += bank.models
        self.eval_calls = []

    def micro_step(self, dt, etime):
        if self.nstep % self.cfg["eval_interval"] != 0:
            return super().micro_step(dt, etime)
        inp = self.micro_step_keeping_input(dt)
        self.evaluator.accumulate(inp, self.coupler)
        if self.domain_eval is not None:
            self.domain_eval.accumulate(inp, self.coupler)
        for _, ce in self.committee_evals:
            ce.accumulate(inp, self.coupler)
        self.eval_calls.append({"step": self.nstep, "etime": etime})

    def finish(self, steps, yaml_path):
        info, evaluator, domain_eval = self.info, self.evaluator, self.domain_eval
        rep = evaluator.report() if self.eval_calls else {}
        drep = None if domain_eval is None else (domain_eval.report() if self.eval_calls else {})
        doc = evaluation_document(info["experiment"], yaml_path, self.cfg["eval_interval"], steps, evaluator, self.eval_models, self.eval_calls,
                                  rep, self.committee_evals, self.eval_domain, domain_eval, drep)
        if self.committee_evals:
            info["committee_reports"] = {d["name"]: d["report"] for d in doc["committees"]}
        if domain_eval is not None:
            info["domain_report"] = drep
        info["surrogate_evaluation"] = os.path.join(os.getcwd(), "surrogate_evaluation.json")
        with open(info["surrogate_evaluation"], "w") as f:
            json.dump(doc, f, indent=1)
        info["surrogate_report"] = rep
        if not self.quiet and rep:
            print(evaluator.table(rep), flush=True)
            if domain_eval is not None:
                print(domain_eval.table(drep), flush=True)
            for c, ce in self.committee_evals:
                print(ce.table(name=c["name"]), flush=True)


def rollout_document(experiment, yaml_path, eval_interval, steps, models, scorer, rep, micro, committees=(), domain_blocks=None,
                     harvest=None, rain_cfg=None, rain=None, water_fixer=None, heat_closure=None):
    """surrogate_rollout.json as a dict.  rep: the scorer's report; domain_blocks: micro.domain_reports() with `training_domain`;
    harvest: harvest_block's result with a harvester; rain_cfg, rain: the checked `surface_rain` and its RainScorer; water_fixer:
    micro.water_fix_reports() with `water_fixer`; heat_closure: micro.heat_closure_reports() with `heat_closure`.  None: no such block."""
    doc = {"experiment": experiment, "yaml": os.path.abspath(yaml_path), "eval_interval": eval_interval, "steps": steps,
           "members": list(scorer.member_names), "models": [dict(m, member=1 + k, form=micro.model_forms[k]) for k, m in enumerate(models)],
           "fields": list(scorer.fields), "statistics": list(rollout.ROLLOUT_STATS), "history": scorer.history,
           "report": rep["times"], "diverged_at": rep["diverged_at"]}
    if committees:
        doc["committees"] = [dict(c, member=scorer.member_names.index(c["name"])) for c in committees]
        for c, g in zip(doc["committees"], micro.guard_reports()):
            if g is not None:
                c["guard"] = g
    if domain_blocks is not None:                                              # one block per network-stepped member
        for entry in doc["models"] + doc.get("committees", []):
            entry["domain"] = domain_blocks[entry["member"]]
    if harvest is not None:
        doc["harvest"] = harvest
    if rain is not None:
        doc["surface_rain"] = dict(rain_cfg, report=rain.times)
    if water_fixer is not None:
        doc["water_fixer"] = water_fixer
    if heat_closure is not None:
        doc["heat_closure"] = heat_closure
    return doc


class RolloutSurrogates(Column):
    fixer_cfg = None                                                           # the checked `water_fixer` key
    closure_cfg = None                                                         # the checked `heat_closure` key

    def configure(self, cfg, nranks):
        _one_rank("rollout_surrogates", nranks)
        self.harvest = harvest_config(cfg)
        self.rain_cfg = surface_rain_config(cfg)
        self.domain_cfg = training_domain_config(cfg)
        self.committees = committee_config(cfg)
        cfg["surrogate_models"], cfg["eval_interval"], cfg["persistence_member"], cfg["nens"] = rollout_config(cfg)
        stepped = [m["name"] for m in cfg["surrogate_models"]] + [c["name"] for c in self.committees]
        self.fixer_cfg = water_fixer_config(cfg, stepped)
        self.closure_cfg = heat_closure_config(cfg, ["kessler"] + stepped, stepped)

    def make_micro(self):
        models = self.cfg["surrogate_models"]
        micro = rollout.Microphysics_Rollout()
        bank = mlp.load_surrogate_bank(models)
        self.stencil = {m["name"]: int(w[0].shape[0]) == 9 for m, w in zip(models, bank)}      # a stencil model reads the level above
        micro.init(self.coupler, bank, self.cfg["persistence_member"], [m["name"] for m in models],
                   [(c["name"], c["members"], c["guard"]) if "guard" in c else (c["name"], c["members"]) for c in self.committees],
                   domains=mlp.load_training_domains(models, bank))
        return micro

    def setup(self, *args):
        super().setup(*args)
        micro, harvest = self.micro, self.harvest
        self.scorer = rollout.RolloutScorer(micro.member_names)
        self.rain = None
        if self.rain_cfg is not None:
            micro.surface_rain = {}                                            # every member but Kessler from its water budget
            self.rain = rollout.RainScorer(micro.member_names, self.rain_cfg["thresholds_mm_h"], self.rain_cfg["thresholds_mm"])
        if self.domain_cfg is not None:
            micro.training_domain = self.domain_cfg
        if self.fixer_cfg is not None:                                         # (members None: every model and committee member)
            micro.water_fixer = {k: v for k, v in self.fixer_cfg.items() if v is not None}
        if self.closure_cfg is not None:                                       # (lists None: the rollout's defaults)
            micro.heat_closure = {k: v for k, v in self.closure_cfg.items() if v is not None}
        self.harvester = None
        if harvest is not None:
            self.harvester = micro.harvester = rollout.RolloutHarvester()
            outside = {}
            if "outside" in harvest:                                           # each harvested model's own box
                o = harvest["outside"]
                outside = dict(outside=o, boxes=[micro.model_box(n, o["margin"], o["fields"]) for n in harvest["members"]],
                               above=[self.stencil[n] for n in harvest["members"]])
            self.harvester.init(self.coupler, harvest["members"], [micro.member_names.index(n) for n in harvest["members"]], os.getcwd(),
                                harvest["samples_per_step"], harvest["ratio_active"], seed=harvest["seed"],
                                max_rainsplit=harvest["max_rainsplit"], **outside)

    def micro_step(self, dt, etime):
        if self.harvester is not None:
            self.micro.harvest_now, self.micro.harvest_etime = self.nstep % self.harvest["interval"] == 0, etime
        if self.domain_cfg is not None:                                        # the report's pass runs at scoring steps only
            self.micro.domain_now = self.nstep % self.cfg["eval_interval"] == 0
        self.micro.time_step(self.coupler, dt)

    def after_step(self, dt, etime):
        if self.nstep % self.cfg["eval_interval"] != 0:
            return
        scorer, micro, step = self.scorer, self.micro, self.nstep
        before = dict(scorer.diverged_at)
        scorer.accumulate(self.coupler, step, etime + dt)
        micro.guard_record(step, dt)                                           # (the only host read of the guards' counts)
        micro.domain_record(step)                                              # (and of the training-domain report's)
        if self.fixer_cfg is not None:
            micro.water_fix_record(step)                                       # (and of the water fixer's statistics)
        if self.closure_cfg is not None:
            micro.heat_closure_record(step)                                    # (and of the latent-heat closure's)
        if self.rain is not None:
            self.rain.accumulate(self.coupler, micro, step, etime + dt)
        for m, d in scorer.diverged_at.items():                                # the other members do not see it: the run goes on
            if d is not None and before[m] is None and not self.quiet:
                print("rollout_surrogates: member %r is non-finite at step %d" % (m, d["step"]), flush=True)

    def finish(self, steps, yaml_path):
        info, scorer, micro, rain = self.info, self.scorer, self.micro, self.rain
        rep = scorer.report() if scorer.times else {"times": [], "diverged_at": dict(scorer.diverged_at)}
        blocks = micro.domain_reports() if self.domain_cfg is not None else None
        doc = rollout_document(info["experiment"], yaml_path, self.cfg["eval_interval"], steps, self.cfg["surrogate_models"], scorer, rep, micro,
                               self.committees, domain_blocks=blocks, rain_cfg=self.rain_cfg, rain=rain,
                               water_fixer=micro.water_fix_reports() if self.fixer_cfg is not None else None,
                               heat_closure=micro.heat_closure_reports() if self.closure_cfg is not None else None,
                               harvest=harvest_block(self.harvest, self.harvester) if self.harvester is not None else None)
        if blocks is not None:
            info["domain_reports"] = {scorer.member_names[m]: b for m, b in enumerate(blocks) if b is not None}
        if self.harvester is not None:
            info["harvest"] = doc["harvest"]
        if self.fixer_cfg is not None:
            info["water_fixer_report"], info["rain_total"] = doc["water_fixer"], micro.rain_total
        if self.closure_cfg is not None:
            info["heat_closure_report"] = doc["heat_closure"]
        if rain is not None:
            info["surface_rain_report"], info["rain_total"] = rain.times, micro.rain_total
            if self.rain_cfg["map"] and micro.rain_total is not None:          # (nens, ny, nx) fp64, mm since the start of the run
                info["surface_rain_map"] = os.path.join(os.getcwd(), "surrogate_rollout_rain.npy")
                np.save(info["surface_rain_map"], np.ascontiguousarray((1000.0 * micro.rain_total).permute(2, 0, 1).cpu().numpy()))
        info["surrogate_rollout"] = os.path.join(os.getcwd(), "surrogate_rollout.json")
        with open(info["surrogate_rollout"], "w") as f:
            json.dump(doc, f, indent=1, allow_nan=False)
        info["rollout_report"] = rep
        if not self.quiet and scorer.times:
            print(scorer.table(rep), flush=True)
            if rain is not None and rain.times:
                print(rain.table(), flush=True)


EXPERIMENT_CLASSES = {"supercell_example": Column, "community_benchmark": CommunityBenchmark, "simple_city": SimpleCity,
                      "inference_ponni": InferencePonni, "gather_statistics": GatherStatistics, "generate_micro_data": GenerateMicroData,
                      "evaluate_surrogates": EvaluateSurrogates, "rollout_surrogates": RolloutSurrogates}


def run(experiment, yaml_path, max_steps=None, device="cuda:0", quiet=False):
    if experiment not in EXPERIMENTS:
        raise ValueError("unknown experiment %r (one of %s)" % (experiment, ", ".join(EXPERIMENTS)))
    cfg = load_config(yaml_path)
    nranks, myrank, device = _distributed(device)
    exp = EXPERIMENT_CLASSES[experiment]()
    exp.configure(cfg, nranks)
    coupler = _coupler(cfg, device, nranks, myrank, yaml_path)
    dycore = Dynamics_Euler_Stratified_WenoFV()
    info = {"experiment": experiment, "nranks": nranks}
    t_main = time.perf_counter()
    exp.setup(cfg, coupler, dycore, info, device, quiet)
    if exp.timed:
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
    etime, steps = _time_loop(cfg, dycore, coupler, exp.step, max_steps)
    if exp.timed:
        torch.cuda.synchronize(device)
        info["simulation_loop_s"] = time.perf_counter() - t0
    exp.finish(steps, yaml_path)
    torch.cuda.synchronize(device)
    info.update(etime=etime, steps=steps, main_s=time.perf_counter() - t_main, dycore_etime=dycore.etime, num_out=dycore.num_out)
    if not quiet and coupler.is_mainproc():
        print("driver %s: %d steps, etime %.6f s, wall %.3f s%s" % (experiment, steps, etime, info["main_s"],
              (", simulation_loop %.3f s" % info["simulation_loop_s"]) if "simulation_loop_s" in info else ""), flush=True)
    return coupler, dycore, info


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("experiment", choices=EXPERIMENTS)
    ap.add_argument("yaml")
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if not os.path.exists(a.yaml):
        print("ERROR: Must pass the input YAML filename as a parameter", file=sys.stderr)       # driver.cpp:21
        return 2
    run(a.experiment, a.yaml, a.max_steps, a.device)
    return 0


if __name__ == "__main__":
    sys.exit(main())
