"""Candidate surrogates rolled out as ensemble members beside Kessler (no reference counterpart; the sample files are those of
experiments/supercell_kessler_surrogate/custom_modules/generate_micro_surrogate_data.h:17-33, the thresholds its :58-62):

  Microphysics_Rollout       one microphysics step that treats every ensemble member differently (mw_member_*, SurrogateBank)
  kessler_members_teacher    mw_kessler_members_teacher: what Kessler would do to each member's own state
  RolloutHarvester           (state, label) samples of the teacher on the model members' states, one file per member
  member_divergence, rollout_report, RolloutScorer    mw_member_divergence and its reports
  member_column_water, member_surface_rain            every member's surface rain from its column water budget
  member_rain_table, rain_report, RainScorer          its contingency table against the Kessler member and the reports
  member_water_fix, water_fix_report                  the water fixer: a member gives back the water its model made
  member_heat_closure, heat_closure_report            the latent-heat closure: a member's temp from its own vapour change
  domain_report                                       a member's cells outside its model's training box, per scoring step"""
import ctypes as C
import os

import numpy as np
import torch

from . import capi
from ._ffi import StatsAndCounts, _field_ptr_array, _ptr, _stream_ptr, grown_workspace
from .capi import check
from .coupler import endrun
from .microphysics import (CP_D, LV, Microphysics_Kessler, column_water, heat_closure_finish, members_copy, surface_rain_finish, water_fix_finish,
                           water_fix_tolerance)
from .mlp import IN5, OUT4, as_surrogate_model
from .ncio import sample_file_append, sample_file_create
from .sampling import sample_buffers, sample_thresholds
from .surrogate_eval import (DOMAIN_CLASSES, CommitteeGuard, SurrogateBank, box_json, domain_box, domain_config, finite_or_none, guard_config,  # noqa: F401
                             json_safe, member_domain, or_dash, skill_cell)

ROLLOUT_FIELDS = ("density_dry", "uvel", "vvel", "wvel", "temp", "water_vapor", "cloud_liquid", "precip_liquid")
ROLLOUT_STATS = ("sum_d", "sum_abs_d", "sum_d2", "max_abs_d", "sum_x", "min_x", "max_x")
ROLLOUT_WATER = ("water_vapor", "cloud_liquid", "precip_liquid")
GUARD_FIELDS = OUT4               # the order of a guard's four thresholds
ROLLOUT_IN5 = IN5                 # fields5 of members_apply and of the teacher


def rollout_member_names(model_names, persistence=True, committees=()):
    """The fixed roles of a rollout's ensemble members: member 0 is Kessler, members 1 .. K the models of the list in its order, then one
    member per committee (names of `committees`, in its order), an optional last member persistence (no microphysics).  More members than
    the dycore steps in one call is an error that names the limit."""
    names = [str(n) for n in model_names]
    if len(set(names)) != len(names) or {"kessler", "persistence"} & set(names):
        endrun("rollout: model names must be unique and neither 'kessler' nor 'persistence'")
    cnames = [str(n) for n in committees]
    if len(set(cnames)) != len(cnames) or ({"kessler", "persistence"} | set(names)) & set(cnames):
        endrun("rollout: committee names must be unique and neither a model's name nor 'kessler' nor 'persistence'")
    members = ["kessler"] + names + cnames + (["persistence"] if persistence else [])
    if len(members) > capi.MW_ROLLOUT_MAX_MEMBERS:
        endrun("rollout: %d models%s%s beside Kessler are %d ensemble members, the dycore steps at most %d"
               % (len(names), (", %d committees" % len(cnames)) if cnames else "", " and persistence" if persistence else "", len(members),
                  capi.MW_ROLLOUT_MAX_MEMBERS))
    return members


class Microphysics_Rollout(Microphysics_Kessler):
    """One microphysics step that treats every ensemble member differently (no reference counterpart): member 0 is stepped by Kessler,
    member k by model k - 1 of `models` (its output written back: Microphysics_Kessler_Surrogate.online for that member), the optional last
    member by nothing.  The dycore, the sponge and the nudger step the members independently, so one run shows how each candidate behaves
    once its own output is fed back.  Kessler runs on member 0 ALONE, extracted to contiguous arrays: its rain sub-cycle count is a minimum
    over all the columns of a call.  Without `surface_rain`, `precl` is written for member 0 only and the other members' precl keeps
    whatever it held.  With `surface_rain` set to a mapping, every budget member's precl is what the step removed from its column's water
    (mw_member_surface_rain: signed, m of water / s; the persistence member gets exactly +0.0) and `rain_total`, (ny, nx, nens) in
    metres, accumulates dt * precl of every member -- Kessler's own precl for member 0.  The mapping may hold `budget_members`, the
    members' names (default: every member but kessler; with kessler in it the budget overwrites Kessler's own precl of member 0, which
    is the closure check of DESIGN.md 13.8).  The step itself is the same either way: the budget only reads the state.
    With `water_fixer` set to a mapping ({members: names, tolerance: 0.0}; members default: every model and committee member; kessler and
    persistence are refused) the step ends with mw_member_water_fix in place of mw_member_surface_rain: a fixed member's column that holds
    more water than before the step is scaled back to what it held (the three water fields only: a mass fixer, no latent heat), the fixed
    members are budget members beside surface_rain's, and rain_total exists with or without surface_rain.  Every other member keeps the
    bits it has without the option.  water_fix_record / water_fix_reports keep the per-step statistics.
    With `heat_closure` set to a mapping ({members: names, closed: names, tolerance: 0.0}; members default: every member but persistence;
    closed default: every model and committee member, a subset of members; kessler and persistence are refused in closed) the step first
    copies temp and water_vapor of the diagnosed members aside and, after the banks, the committees and the guard's commit and BEFORE the
    water fixer, calls mw_member_heat_closure: every diagnosed member's residual r = temp - (temp_before + (lv / cp_d) (rho_v_before -
    rho_v) / rho_d) is measured and a closed member's temp becomes the diagnosed value where |r| > tolerance.  Only temp is written, and
    only in closed members.  heat_closure_record / heat_closure_reports keep the per-step statistics.
    With a `harvester` (RolloutHarvester) and `harvest_now` set, the step harvests Kessler labels on the model members' own states
    between the Kessler member's step and the models'; harvesting reads the state and never writes it.
    With `training_domain` (surrogate_eval.domain_config's mapping, or True) and `domain_now` set, the step counts, for every model member
    and every committee member, the cells of its five input fields that lie outside the box of its model's (its committee's) input
    scaling rows -- one mw_member_domain call with every slot -1 at the harvest's place in the step, after the Kessler
    member's step and before members_apply, so it sees the state the networks are about to replace.  It only reads.  A guarded member
    listed there gets its flag bytes written NOT in that call but in the guards' own call, in the guard's position of the step (after
    the loop of committee_guard_flag, before the commit); a committee member's state is the same at both points, so the bits are too."""

    mlp_strict = 0        # 1: the thread-per-cell MLP kernels (mw_mlp_set_strict)
    harvester = None      # a RolloutHarvester: time_step harvests when harvest_now is set (the driver sets it, and harvest_etime, per step)
    harvest_now = False
    harvest_etime = 0.0
    surface_rain = None   # a mapping (may be empty; key budget_members): precl of the budget members and rain_total from the water budget
    _w_before = None
    rain_total = None     # with surface_rain: (ny, nx, nens) fp64, metres of water since the first step with the option
    water_fixer = None    # a mapping (keys members, tolerance): a fixed member's column that gained water is scaled back
    _water_fix = None     # with water_fixer: the StatsAndCounts of the last step, on the device
    _water_fix_fresh = False
    _water_fix_for = None
    _water_fix_steps = ()
    heat_closure = None   # a mapping (keys members, closed, tolerance): a closed member's temp follows from its own vapour change
    _heat = None          # with heat_closure: the StatsAndCounts of the last step, on the device
    _heat_fresh = False
    _heat_for = None
    _heat_steps = ()
    _heat_before = None   # the two scratch fields: temp and water_vapor of the diagnosed members before the step
    training_domain = None   # None, True or a domain_config mapping: time_step counts the cells outside the box when domain_now is set
    domain_now = False       # (the driver sets it at scoring steps)
    _domains = None          # per model None or its training-domain table (init's `domains`): the rows domain_box reads

    def micro_name(self):
        return "rollout"

    def init(self, coupler, models, persistence=True, names=None, committees=(), domains=None):
        """models: (W1, b1, W2, b2, scl_in, scl_out) tuples as load_surrogate_weights returns them (the state form) or SurrogateModel
        tuples with the form last (load_surrogate_model), single-cell and stencil networks and both forms in any order (self.model_forms: the
        forms by name, in the models' order); names: theirs (default model0, model1, ...).  committees: (name, [model names]) pairs; each is one more member after the
        models, replaced in place from its OWN state by the mean of its models (1 .. 16 of one width, SurrogateBank.committee_apply on that
        width's bank).  A third entry, (name, [model names], guard), makes the committee a GUARDED one (guard: surrogate_eval.guard_config's
        mapping of thresholds and max_rainsplit): its member is the committee's mean where its models agree and Kessler on the columns
        where they do not (SurrogateBank.committee_guard_apply's step).  A guard with `domain` also hands Kessler the columns that
        hold a cell outside the box of the committee's models (domain_box with the guard's margin and fields); all such members go
        into ONE mw_member_domain call per step, after the loop of committee_guard_flag.  All guarded members share one scratch
        (CommitteeGuard) and one columns-teacher call per step, so they share one max_rainsplit; every other member keeps the bits it has
        without the guard.
        domains: None, or per model None or its training-domain table (mlp.load_training_domain), handed to every
        domain_box this object calls -- the report's boxes and the domain guards' -- in place of the model's scaling rows.
        The coupler must have 1 + len(models) + len(committees) (+ 1 with persistence) members."""
        models = [as_surrogate_model(m) for m in models]
        self.model_forms = [m.form for m in models]
        names = ["model%d" % k for k in range(len(models))] if names is None else [str(n) for n in names]
        if len(names) != len(models):
            endrun("Microphysics_Rollout: %d names for %d models" % (len(names), len(models)))
        guards = [guard_config(c[2], "the guard of committee %r" % str(c[0])) if len(c) > 2 and c[2] is not None else None for c in committees]
        if len({g["max_rainsplit"] for g in guards if g is not None}) > 1:
            endrun("Microphysics_Rollout: the guarded committees share one columns-teacher call per step: give them one max_rainsplit")
        committees = [(str(c[0]), [str(n) for n in c[1]]) for c in committees]
        self.member_names = rollout_member_names(names, persistence, [c[0] for c in committees])
        self.persistence = bool(persistence)
        if coupler.get_nens() != len(self.member_names):
            endrun("Microphysics_Rollout: %d models%s%s beside Kessler need nens = %d, the coupler has %d"
                   % (len(models), (", %d committees" % len(committees)) if committees else "", " and persistence" if persistence else "",
                      len(self.member_names), coupler.get_nens()))
        for cname, cmodels in committees:
            if not 1 <= len(cmodels) <= capi.MW_COMMITTEE_MAX_MODELS:
                endrun("Microphysics_Rollout: committee %r has %d models, a committee has 1 to %d" % (cname, len(cmodels), capi.MW_COMMITTEE_MAX_MODELS))
            if len(set(cmodels)) != len(cmodels) or any(n not in names for n in cmodels):
                endrun("Microphysics_Rollout: committee %r must name distinct models of the list (%s)" % (cname, ", ".join(names)))
            if len({int(np.shape(models[names.index(n)][0])[0]) for n in cmodels}) != 1:
                endrun("Microphysics_Rollout: committee %r mixes single-cell and stencil models: a committee has one width" % cname)
        super().init(coupler)
        coupler.set_option("micro", "rollout")
        widths = []
        for m in models:
            if int(np.shape(m[0])[0]) not in widths:
                widths.append(int(np.shape(m[0])[0]))
        # one bank per width; a model keeps the member its place in the list gives it
        self.banks = [(SurrogateBank([m for m in models if np.shape(m[0])[0] == w], coupler.device),
                       [1 + k for k, m in enumerate(models) if np.shape(m[0])[0] == w]) for w in widths]
        # a committee runs on its width's bank: (bank, its models' places in that bank, its member)
        self.committees = []
        for ci, (cname, cmodels) in enumerate(committees):
            w = int(np.shape(models[names.index(cmodels[0])][0])[0])
            in_bank = [k for k, m in enumerate(models) if np.shape(m[0])[0] == w]
            self.committees.append((self.banks[widths.index(w)][0], [in_bank.index(names.index(n)) for n in cmodels], 1 + len(models) + ci))
        self.guards = guards                                                   # per committee: the checked guard or None
        self._models, self._model_names, self._committee_names = models, names, committees
        if domains is not None and len(domains) != len(models):
            endrun("Microphysics_Rollout: %d domains for %d models (one per model, None where it has none)" % (len(domains), len(models)))
        self._domains = None if domains is None else list(domains)
        # per committee: the box of a guard with `domain` (refused here, before any step, when the models' ranges do not intersect)
        self._guard_boxes = [self._committee_box(ci, g["domain"]) if g is not None and "domain" in g else None for ci, g in enumerate(guards)]
        self._guard_domain_counts = None                                       # device (domain-guarded members, 16) of the last step
        self._domain = None                                                    # the report's (cfg, members, boxes), made at its first step
        self._domain_counts = self._domain_fresh = None
        self._domain_steps = []                                                # per domain_record: (step, host counts (members, 16))
        self._domain_cells = (None, None)                                      # a member's cells and columns, known at the first step
        self._guard = None                                                     # the CommitteeGuard all guarded members share
        self._guard_steps = [[] for _ in committees]
        self._m0 = None
        self._w_before = self.rain_total = None
        self._water_fix, self._water_fix_fresh, self._water_fix_for, self._water_fix_steps = None, False, None, []
        self._heat, self._heat_fresh, self._heat_for, self._heat_steps, self._heat_before = None, False, None, [], None

    def time_step(self, coupler, dt):
        dm = coupler.get_data_manager_readwrite()
        temp, rho_d = dm.get("temp"), dm.get("density_dry", readonly=True)
        rho_v, rho_c, rho_r, precl = dm.get("water_vapor"), dm.get("cloud_liquid"), dm.get("precip_liquid"), dm.get("precl")
        nz, nens = coupler.get_nz(), coupler.get_nens()
        ncol = coupler.get_ny() * coupler.get_nx()
        n = nz * ncol
        self._domain_cells = (n, ncol)
        L = capi.lib()
        if self._m0 is None or self._m0[0][0].numel() != n or self._m0[1].numel() != ncol:
            self._m0 = ([torch.empty(n, dtype=torch.float64, device=coupler.device) for _ in range(5)],
                        torch.empty(ncol, dtype=torch.float64, device=coupler.device))
        (v0, c0, r0, d0, t0), p0 = self._m0
        ws = grown_workspace(self, "_ws", L.mw_kessler_workspace_bytes(nz, ncol), coupler.device)
        st = _stream_ptr(coupler.device)
        closure = self._closure_setup()
        if closure is not None:                                                # temp and water_vapor of the diagnosed members, before anything is stepped
            if self._heat_before is None or self._heat_before[0].shape != temp.shape or self._heat_before[0].device != temp.device:
                self._heat_before = [torch.empty_like(temp), torch.empty_like(temp)]
            members_copy(n, nens, closure[0], [temp, rho_v], self._heat_before)
        fixer = self._fixer_setup()
        budget = self._budget_members(coupler, None if fixer is None else fixer[0])
        if budget is not None:                                                 # W_before of ALL members, before anything is stepped
            self._w_before = column_water([rho_v, rho_c, rho_r], nz, ncol, nens, coupler.get_dz(), self._w_before)
        check(L.mw_kessler_set_strict(self.strict))
        with torch.cuda.device(coupler.device):
            check(L.mw_member_extract(n, nens, 0, 5, _field_ptr_array([rho_v, rho_c, rho_r, rho_d, temp]), _field_ptr_array([v0, c0, r0, d0, t0]), st))
            check(L.mw_kessler_time_step(nz, ncol, coupler.get_dz(), float(dt), _ptr(v0), _ptr(c0), _ptr(r0), _ptr(d0), _ptr(t0), _ptr(p0),
                                         _ptr(ws), None, st))
            check(L.mw_member_insert(n, nens, 0, 4, _field_ptr_array([v0, c0, r0, t0]), _field_ptr_array([rho_v, rho_c, rho_r, temp]), st))
            check(L.mw_member_insert(ncol, nens, 0, 1, _field_ptr_array([p0]), _field_ptr_array([precl]), st))
        if self.harvester is not None and self.harvest_now:                    # the teacher sees the state each model is about to replace
            self.last_harvest = self.harvester.harvest(coupler, dt, self.harvest_etime)
        if self.training_domain is not None and self.domain_now:               # (it sees that state too, and only reads it)
            _, members, boxes = self._domain_setup()
            self._domain_counts = member_domain(nz, [temp, rho_d, rho_v, rho_c, rho_r], members, boxes, self._domain_counts)
            self._domain_fresh = True
        for bank, members in self.banks:
            bank.strict = self.mlp_strict
            bank.members_apply(nz, members, [temp, rho_d, rho_v, rho_c, rho_r])
        guards = getattr(self, "guards", None) or [None] * len(getattr(self, "committees", ()))
        guarded = [ci for ci, g in enumerate(guards) if g is not None]
        in5 = [temp, rho_d, rho_v, rho_c, rho_r]
        if guarded and self._guard is None:
            self._guard = CommitteeGuard(temp, nz, len(guarded))
        for ci, (bank, sel, member) in enumerate(getattr(self, "committees", ())):
            bank.strict = self.mlp_strict
            if guards[ci] is None:
                bank.committee_apply(nz, sel, member, in5, [temp, rho_v, rho_c, rho_r])
            else:                                                              # mean, range and flags of this member; the state is not written yet
                bank.committee_guard_flag(nz, sel, member, in5, [guards[ci][f] for f in GUARD_FIELDS], self._guard, guarded.index(ci))
        boxed = [ci for ci in guarded if self._guard_boxes[ci] is not None]
        if boxed:                                                              # every domain-guarded member in one call, flags into its slot
            self._guard_domain_counts = member_domain(nz, in5, [self.committees[ci][2] for ci in boxed], [self._guard_boxes[ci] for ci in boxed],
                                                      self._guard_domain_counts, self._guard, [guarded.index(ci) for ci in boxed])
        if guarded:                                                            # Kessler on every flagged column, then the guarded members' commit
            self._guard.commit(nz, [self.committees[ci][2] for ci in guarded], in5, guards[guarded[0]]["max_rainsplit"], coupler.get_dz(), dt)
        if closure is not None:                                                # the vapour change is the network's: before the fixer
            self._heat = heat_closure_finish(temp, rho_d, rho_v, self._heat_before, nz, ncol, nens, closure[0], closure[1], closure[2],
                                             coupler.get_dz(), dt, holder=self)
            self._heat_fresh = True
        if fixer is not None:                                                  # the budget, and the fixed members give back the water they made
            self._water_fix = water_fix_finish([rho_v, rho_c, rho_r], nz, ncol, nens, budget, range(nens), fixer[0], fixer[1], coupler.get_dz(),
                                               dt, self._w_before, precl, self.rain_total, holder=self)
            self._water_fix_fresh = True
        elif budget is not None:
            surface_rain_finish([rho_v, rho_c, rho_r], nz, ncol, nens, budget, range(nens), coupler.get_dz(), dt, self._w_before, precl,
                                self.rain_total)

    def _fixer_setup(self):
        """None without `water_fixer`; else (the fixed members' indices, the tolerance), checked."""
        wf = self.water_fixer
        if wf is None:
            return None
        if not hasattr(wf, "keys") or set(wf.keys()) - {"members", "tolerance"}:
            endrun("Microphysics_Rollout: water_fixer is None or a mapping whose keys are members and tolerance")
        stepped = self.member_names[1:len(self.member_names) - int(self.persistence)]      # models and committees: what a network steps
        names = wf.get("members")
        names = list(stepped) if names is None else [str(m) for m in names]
        if len(set(names)) != len(names) or any(m not in stepped for m in names):
            endrun("Microphysics_Rollout: water_fixer's members must be distinct network-stepped members (%s), never kessler or persistence"
                   % ", ".join(stepped))
        try:
            tolerance = water_fix_tolerance(wf.get("tolerance", 0.0), "water_fixer.tolerance")
        except ValueError as err:
            endrun("Microphysics_Rollout: " + str(err))
        if self._water_fix_for is not wf:                                      # another configuration: its own records
            self._water_fix_for, self._water_fix_steps, self._water_fix, self._water_fix_fresh = wf, [], None, False
        return [self.member_names.index(m) for m in names], tolerance

    def water_fix_record(self, step):
        """At a scoring step, after a time_step with `water_fixer`: fetches that step's statistics of every member (the only host read of
        them; no other step synchronises for the report)."""
        if self.water_fixer is None or not self._water_fix_fresh:
            return
        stats, counts = self._water_fix.host()
        self._water_fix_steps.append((int(step), counts.reshape(-1, 2), stats.reshape(-1, 2)))
        self._water_fix_fresh = False

    def water_fix_reports(self):
        """None without `water_fixer`; else the `water_fixer` block of surrogate_rollout.json (water_fix_report) from the recorded steps."""
        fixer = self._fixer_setup()
        if fixer is None:
            return None
        return water_fix_report(self.member_names, fixer[0], fixer[1], self._domain_cells[1], self._water_fix_steps)

    def _closure_setup(self):
        """None without `heat_closure`; else (the diagnosed members' indices, the closed members' indices, the tolerance), checked."""
        hc = self.heat_closure
        if hc is None:
            return None
        if not hasattr(hc, "keys") or set(hc.keys()) - {"members", "closed", "tolerance"}:
            endrun("Microphysics_Rollout: heat_closure is None or a mapping whose keys are members, closed and tolerance")
        stepped = self.member_names[1:len(self.member_names) - int(self.persistence)]      # models and committees: what a network steps
        every = self.member_names[:len(self.member_names) - int(self.persistence)]
        names = hc.get("members")
        names = list(every) if names is None else [str(m) for m in names]
        if not names or len(set(names)) != len(names) or any(m not in self.member_names for m in names):
            endrun("Microphysics_Rollout: heat_closure's members must be one or more distinct members (%s)" % ", ".join(self.member_names))
        closed = hc.get("closed")
        closed = [m for m in stepped if m in names] if closed is None else [str(m) for m in closed]
        if len(set(closed)) != len(closed) or any(m not in stepped for m in closed):
            endrun("Microphysics_Rollout: heat_closure's closed must be distinct network-stepped members (%s), never kessler or persistence"
                   % ", ".join(stepped))
        if any(m not in names for m in closed):
            endrun("Microphysics_Rollout: heat_closure's closed members must be among its members (%s)" % ", ".join(names))
        try:
            tolerance = water_fix_tolerance(hc.get("tolerance", 0.0), "heat_closure.tolerance")
        except ValueError as err:
            endrun("Microphysics_Rollout: " + str(err))
        if self._heat_for is not hc:                                           # another configuration: its own records
            self._heat_for, self._heat_steps, self._heat, self._heat_fresh = hc, [], None, False
        return [self.member_names.index(m) for m in names], [self.member_names.index(m) for m in closed], tolerance

    def heat_closure_record(self, step):
        """At a scoring step, after a time_step with `heat_closure`: fetches that step's statistics of every member (the only host read of
        them; no other step synchronises for the report)."""
        if self.heat_closure is None or not self._heat_fresh:
            return
        stats, counts = self._heat.host()
        self._heat_steps.append((int(step), counts.reshape(-1, 2), stats.reshape(-1, 6)))
        self._heat_fresh = False

    def heat_closure_reports(self):
        """None without `heat_closure`; else the `heat_closure` block of surrogate_rollout.json (heat_closure_report) from the recorded steps."""
        closure = self._closure_setup()
        if closure is None:
            return None
        return heat_closure_report(self.member_names, closure[0], closure[1], closure[2], self._domain_cells[0], self._domain_cells[1],
                                   self._heat_steps)

    def _budget_members(self, coupler, fixed=None):
        """None without `surface_rain` and without a fixer (fixed: None or its members' indices); else the budget members' indices --
        surface_rain's, then the fixed ones that are not among them -- with rain_total and the W_before buffer in place."""
        sr = self.surface_rain
        if sr is None and fixed is not None:
            sr = {"budget_members": []}
        if sr is None:
            return None
        if not hasattr(sr, "keys") or set(sr.keys()) - {"budget_members"}:
            endrun("Microphysics_Rollout: surface_rain is None or a mapping whose only key is budget_members")
        names = sr.get("budget_members")
        names = [m for m in self.member_names if m != "kessler"] if names is None else [str(m) for m in names]
        if len(set(names)) != len(names) or any(m not in self.member_names for m in names):
            endrun("Microphysics_Rollout: surface_rain's budget_members must be distinct members (%s)" % ", ".join(self.member_names))
        shape = (coupler.get_ny(), coupler.get_nx(), coupler.get_nens())
        if self.rain_total is None or tuple(self.rain_total.shape) != shape:
            self.rain_total = torch.zeros(shape, dtype=torch.float64, device=coupler.device)
            self._w_before = None
        budget = [self.member_names.index(m) for m in names]
        return budget + [m for m in (fixed or ()) if m not in budget]

    def _committee_box(self, ci, cfg):
        cname, cmodels = self._committee_names[ci]
        places = [self._model_names.index(n) for n in cmodels]
        return domain_box([self._models[k] for k in places], cfg["margin"], cfg["fields"], names=cmodels, tables=self._tables(places))

    def _tables(self, places):
        return None if self._domains is None else [self._domains[k] for k in places]

    def model_box(self, name, margin=0.0, fields=IN5):
        """domain_box of the model called `name` alone, from its training-domain table where it has one."""
        k = self._model_names.index(str(name))
        return domain_box([self._models[k]], margin, fields, names=[str(name)], tables=self._tables([k]))

    def _domain_setup(self):
        """(the checked training_domain, the network-stepped members, their boxes (members, 5, 2)): every model member with its model's
        box, every committee member with its committee's."""
        if self._domain is None or self._domain[3] is not self.training_domain:
            cfg = domain_config(self.training_domain, "training_domain")
            boxes = [self.model_box(n, cfg["margin"], cfg["fields"]) for n in self._model_names]
            boxes += [self._committee_box(ci, cfg) for ci in range(len(self._committee_names))]
            if not boxes or len(boxes) > capi.MW_DOMAIN_MAX_MEMBERS:
                endrun("Microphysics_Rollout: training_domain reports 1 to %d network-stepped members, this rollout has %d"
                       % (capi.MW_DOMAIN_MAX_MEMBERS, len(boxes)))
            self._domain = (cfg, list(range(1, 1 + len(boxes))), np.stack(boxes), self.training_domain)
            self._domain_counts, self._domain_steps = None, []
        return self._domain[:3]

    def domain_record(self, step):
        """At a scoring step, after a time_step with domain_now set: fetches that step's counts of every reported member (the only host
        read of them; no other step synchronises for the report)."""
        if self.training_domain is None or not self._domain_fresh:
            return
        self._domain_steps.append((int(step), self._domain_counts.cpu().numpy().copy()))
        self._domain_fresh = False

    def domain_reports(self):
        """Per member, in member_names' order: None (kessler, persistence, or no training_domain), or the member's `domain` block of
        surrogate_rollout.json (domain_report)."""
        out = [None] * len(self.member_names)
        if self.training_domain is None:
            return out
        cfg, members, boxes = self._domain_setup()
        cells, ncol = self._domain_cells
        for j, m in enumerate(members):
            out[m] = domain_report(cfg, boxes[j], cells, ncol, [(step, counts[j]) for step, counts in self._domain_steps])
        return out

    def guard_record(self, step, dt):
        """At a scoring step, after time_step: fetches every guarded member's flagged columns and rain sub-cycle count of that step (the only
        host read of them; no other step synchronises for the guards), and with a `domain` in the guard its outside columns."""
        guarded = [ci for ci, g in enumerate(getattr(self, "guards", ())) if g is not None]
        if not guarded or self._guard is None:
            return
        counts, rs = self._guard.read(dt, [self.committees[ci][2] for ci in guarded])
        boxed = [ci for ci in guarded if self._guard_boxes[ci] is not None]
        outside = self._guard_domain_counts[:, 15].cpu().tolist() if boxed and self._guard_domain_counts is not None else []
        for slot, ci in enumerate(guarded):
            self._guard_steps[ci].append({"step": int(step), "flagged": counts[slot][0], "rainsplit": rs[slot], "flagged_total": counts[slot][1]})
            if ci in boxed and outside:
                self._guard_steps[ci][-1]["outside_columns"] = int(outside[boxed.index(ci)])

    def guard_reports(self):
        """Per committee, in the list's order: None, or the guarded member's `guard` block of surrogate_rollout.json -- thresholds (inf as the
        string "inf"), max_rainsplit, columns, flagged_total (the device accumulator at the last scoring step), and steps: {step, flagged,
        rainsplit} per scoring step (rainsplit 0: the Kessler part was skipped).  A guard with `domain` adds domain: {margin, fields, box}
        and outside_columns to every step; flagged stays the union of both criteria, from the guard's count word."""
        out = []
        for ci, g in enumerate(getattr(self, "guards", ())):
            if g is None:
                out.append(None)
                continue
            steps = self._guard_steps[ci]
            out.append({"thresholds": {f: json_safe(g[f]) for f in GUARD_FIELDS}, "max_rainsplit": g["max_rainsplit"],
                        "columns": self._guard.ncol if self._guard is not None else None,
                        "flagged_total": steps[-1]["flagged_total"] if steps else 0,
                        "steps": [{k: s[k] for k in ("step", "flagged", "rainsplit", "outside_columns") if k in s} for s in steps]})
            if "domain" in g:
                out[-1]["domain"] = dict(g["domain"], box=box_json(self._guard_boxes[ci]))
        return out


def water_fix_report(member_names, fixed, tolerance, columns, records):
    """The `water_fixer` block of surrogate_rollout.json from raw arrays -- pure numpy.  member_names: the rollout's; fixed: the fixed
    members' indices; columns: a member's columns; records: (step, counts (nens, 2) int64 = fixed and skipped columns, stats (nens, 2) fp64 =
    sum and max of the excess, kg / m^2) per scoring step, mw_member_water_fix's outputs.  Returns tolerance, members (names), columns,
    steps: {step, members: {name: {columns_fixed, columns_skipped, water_removed_kg_m2: {mean, max}}}} with the mean over ALL the member's
    columns, and totals per member over the recorded steps: the counts summed, water_removed_kg_m2 {mean: the steps' means summed -- what a
    column lost to the fixer on average over those steps -- and max}."""
    nens = len(member_names)
    fixed = [int(m) for m in fixed]
    if any(not 0 <= m < nens for m in fixed) or len(set(fixed)) != len(fixed):
        endrun("water_fix_report: the fixed members must be distinct indices of the member names")
    columns = None if columns is None else int(columns)
    steps = []
    totals = {member_names[m]: {"columns_fixed": 0, "columns_skipped": 0, "water_removed_kg_m2": {"mean": 0.0, "max": 0.0}} for m in fixed}
    for step, counts, stats in records:
        counts, stats = np.asarray(counts, dtype=np.int64), np.asarray(stats, dtype=np.float64)
        if counts.shape != (nens, 2) or stats.shape != (nens, 2):
            endrun("water_fix_report: (%d, 2) counts and (%d, 2) statistics per step expected" % (nens, nens))
        row = {}
        for m in fixed:
            mean = float(stats[m, 0]) / columns if columns else None
            row[member_names[m]] = {"columns_fixed": int(counts[m, 0]), "columns_skipped": int(counts[m, 1]),
                                    "water_removed_kg_m2": {"mean": mean, "max": float(stats[m, 1])}}
            t = totals[member_names[m]]
            t["columns_fixed"] += int(counts[m, 0])
            t["columns_skipped"] += int(counts[m, 1])
            if mean is not None:
                t["water_removed_kg_m2"]["mean"] += mean
            t["water_removed_kg_m2"]["max"] = max(t["water_removed_kg_m2"]["max"], float(stats[m, 1]))
        steps.append({"step": int(step), "members": row})
    return {"tolerance": float(tolerance), "members": [member_names[m] for m in fixed], "columns": columns, "steps": steps, "totals": totals}


def heat_closure_report(member_names, members, closed, tolerance, cells, columns, records, lv=LV, cp_d=CP_D):
    """The `heat_closure` block of surrogate_rollout.json from raw arrays -- pure numpy.  member_names: the rollout's; members / closed: the
    diagnosed and the closed members' indices (closed a subset of members); cells / columns: a member's cells (nz * ny * nx) and columns;
    records: (step, counts (nens, 2) int64 = closed and skipped cells, stats (nens, 6) fp64 = sum r, sum |r|, sum r^2, max |r|, sum H,
    max |H|) per scoring step, mw_member_heat_closure's outputs.  Returns lv, cp_d, tolerance, members, closed (names), cells, columns,
    steps: {step, members: {name: {cells_closed, cells_skipped, residual_K: {bias, mae, rmse, max}, heating_W_m2: {mean, max}}}} -- bias, mae
    and rmse over the member's cells that were not skipped (None when there is none), the mean of the heating over ALL the member's
    columns -- and totals per member over the recorded steps: the counts summed, residual_K {bias, mae, rmse over all the steps' cells, max},
    heating_W_m2 {mean: the mean of the steps' means, max}."""
    nens = len(member_names)
    members, closed = [int(m) for m in members], [int(m) for m in closed]
    if any(not 0 <= m < nens for m in members) or len(set(members)) != len(members):
        endrun("heat_closure_report: the diagnosed members must be distinct indices of the member names")
    if any(m not in members for m in closed) or len(set(closed)) != len(closed):
        endrun("heat_closure_report: the closed members must be distinct members of the diagnosed ones")
    cells = None if cells is None else int(cells)
    columns = None if columns is None else int(columns)

    def residual(n, s, a, q, mx):
        return {"bias": s / n if n else None, "mae": a / n if n else None, "rmse": float(np.sqrt(q / n)) if n else None, "max": mx}

    steps = []
    acc = {m: {"closed": 0, "skipped": 0, "n": 0, "s": 0.0, "a": 0.0, "q": 0.0, "max": 0.0, "h": 0.0, "hmax": 0.0, "steps": 0} for m in members}
    for step, counts, stats in records:
        counts, stats = np.asarray(counts, dtype=np.int64), np.asarray(stats, dtype=np.float64)
        if counts.shape != (nens, 2) or stats.shape != (nens, 6):
            endrun("heat_closure_report: (%d, 2) counts and (%d, 6) statistics per step expected" % (nens, nens))
        row = {}
        for m in members:
            n = (cells - int(counts[m, 1])) if cells is not None else 0
            s, a, q, mx, h, hmax = (float(x) for x in stats[m])
            mean = h / columns if columns else None
            row[member_names[m]] = {"cells_closed": int(counts[m, 0]), "cells_skipped": int(counts[m, 1]), "residual_K": residual(n, s, a, q, mx),
                                    "heating_W_m2": {"mean": mean, "max": hmax}}
            t = acc[m]
            t["closed"] += int(counts[m, 0]); t["skipped"] += int(counts[m, 1]); t["n"] += n; t["steps"] += 1      # noqa: E702
            t["s"] += s; t["a"] += a; t["q"] += q; t["max"] = max(t["max"], mx); t["hmax"] = max(t["hmax"], hmax)  # noqa: E702
            t["h"] += mean if mean is not None else 0.0
        steps.append({"step": int(step), "members": row})
    totals = {member_names[m]: {"cells_closed": t["closed"], "cells_skipped": t["skipped"],
                                "residual_K": residual(t["n"], t["s"], t["a"], t["q"], t["max"]),
                                "heating_W_m2": {"mean": t["h"] / t["steps"] if t["steps"] and columns else None, "max": t["hmax"]}}
              for m, t in acc.items()}
    return {"lv": float(lv), "cp_d": float(cp_d), "tolerance": float(tolerance), "members": [member_names[m] for m in members],
            "closed": [member_names[m] for m in closed], "cells": cells, "columns": columns, "steps": steps, "totals": totals}


def domain_report(cfg, box, cells, columns, records):
    """A member's `domain` block from its raw counts -- pure numpy.  cfg: the checked domain_config; box: its (5, 2) box; cells / columns:
    the member's cells (nz * ny * nx) and columns; records: (step, 16 int64 words of mw_member_domain) per scoring step.  Returns margin,
    fields, box ({field: [lo, hi]}, inf as a string), cells, columns, first_outside_step (the first recorded step with an outside column,
    None if never) and steps: {step, outside_columns, below / above / nan: {field: cells}} over the five fields of IN5."""
    steps, first = [], None
    for step, words in records:
        words = np.asarray(words, dtype=np.int64).reshape(-1)
        if words.shape != (capi.MW_DOMAIN_WORDS,):
            endrun("domain_report: %d count words per member and step expected" % capi.MW_DOMAIN_WORDS)
        row = {"step": int(step), "outside_columns": int(words[15])}
        for c, cname in enumerate(DOMAIN_CLASSES):
            row[cname] = {f: int(words[3 * i + c]) for i, f in enumerate(IN5)}
        steps.append(row)
        if first is None and words[15] > 0:
            first = int(step)
    return {"margin": cfg["margin"], "fields": list(cfg["fields"]), "box": box_json(box), "cells": None if cells is None else int(cells),
            "columns": None if columns is None else int(columns), "first_outside_step": first, "steps": steps}


def kessler_members_teacher(coupler, members, dt, max_rainsplit=64, outs=None, return_rainsplit=False):
    """mw_kessler_members_teacher on the coupler's member-fastest fields: what Kessler would do to the state of every member in `members`,
    each member alone, out of place.  Returns the four teacher tensors (temp, water_vapor, cloud_liquid, precip_liquid after Kessler), each
    (nz, ny, nx, nens); only the listed members' elements are written (outs: four tensors to write into, default new uninitialised ones).
    A member whose own state asks for more than max_rainsplit rain sub-cycles, or whose rain CFL step is not a positive finite number, is
    skipped: not computed, not written.  return_rainsplit=True: (tensors, counts per listed member, 0 = skipped), at the price of a
    stream synchronisation.  The coupler's fields are read only."""
    dm = coupler.get_data_manager_readonly()
    f5 = [dm.get(n, True) for n in ROLLOUT_IN5]
    members = [int(m) for m in members]
    nz, nens = coupler.get_nz(), coupler.get_nens()
    ncol = coupler.get_ny() * coupler.get_nx()
    if outs is None:
        outs = [torch.empty_like(f5[0]) for _ in range(4)]
    if len(outs) != 4 or any(o.shape != f5[0].shape or o.device != f5[0].device for o in outs):
        endrun("kessler_members_teacher: outs must be four tensors of the fields' shape on their device")
    L = capi.lib()
    nbytes = L.mw_kessler_members_teacher_workspace_bytes(nz, ncol, nens)
    if nbytes <= 0:
        endrun("kessler_members_teacher: nz = %d, %d columns and %d members are out of range (nz >= 2, at most 64 members)" % (nz, ncol, nens))
    ws = grown_workspace(coupler, "_ws_teacher", nbytes, coupler.device)
    rs = (C.c_int * max(1, len(members)))()
    with torch.cuda.device(coupler.device):
        check(L.mw_kessler_members_teacher(nz, ncol, nens, len(members), (C.c_int * max(1, len(members)))(*members), coupler.get_dz(), float(dt),
                                           int(max_rainsplit), _field_ptr_array(f5), _field_ptr_array(outs), rs if return_rainsplit else None,
                                           _ptr(ws), _stream_ptr(coupler.device)))
    return (outs, [int(rs[j]) for j in range(len(members))]) if return_rainsplit else outs


SAMPLE_CLASSES = ("outside", "active", "inactive")      # mw_member_sample_mask_domain's classes, in the order of its thresholds and counts


def harvest_thresholds(samples_per_step, ratio_active, prior_active, ncell, share, eligible_outside):
    """(thr_outside, thr_active, thr_inactive) of a harvest with `outside` -- pure Python.  The part `share` of
    samples_per_step is asked of the eligible_outside cells that ARE outside the member's box in this call (a count, not a prior: 0 at
    the start of a rollout, most of the member later); the rest is DataGenerator's two classes at their prior rates, each clamped to 1."""
    inside = (1 - share) * samples_per_step
    thr_act, thr_inact = sample_thresholds(ratio_active * inside, (1 - ratio_active) * inside, prior_active, ncell)
    thr_act, thr_inact = min(1.0, thr_act), min(1.0, thr_inact)
    thr_out = 0.0 if eligible_outside == 0 else min(1.0, share * samples_per_step / eligible_outside)
    return thr_out, thr_act, thr_inact


def member_sample_mask_domain(nz, fields5, teacher4, members, boxes, above, key0, thr, mask=None, counts=None):
    """mw_member_sample_mask_domain on the member-fastest fields5 / teacher4 (each (nz, ..., nens), contiguous fp64, one device): for
    member members[j], its box boxes[j] ((5, 2), domain_box), above[j] (its model reads the level above) and thr[j] = (outside, active,
    inactive) the six counts -- eligible per class of SAMPLE_CLASSES, then taken per class -- and, with `mask` (uint8, one byte per
    element), the taken elements.  Returns the DEVICE int64 tensor (len(members), 6), written into `counts` if given; the call SETs it
    and does not synchronise.  mask=None: count only."""
    members = [int(m) for m in members]
    boxes = np.ascontiguousarray(boxes, dtype=np.float64)
    thr = np.ascontiguousarray(thr, dtype=np.float64)
    nm, f = len(members), fields5[0]
    nens, dev = int(f.shape[-1]), f.device
    if len(fields5) != 5 or len(teacher4) != 4 or any(t.shape != f.shape or t.dtype != torch.float64 or not t.is_contiguous() or t.device != dev
                                                      for t in list(fields5) + list(teacher4)):
        endrun("member_sample_mask_domain: five fields and four teacher values, contiguous float64 of one shape (nz, ..., nens) and device, expected")
    n = f.numel() // nens
    if int(nz) < 1 or n % int(nz) != 0:
        endrun("member_sample_mask_domain: %d cells per member are not a whole number of columns of nz = %d" % (n, nz))
    if not 1 <= nm <= capi.MW_DOMAIN_MAX_MEMBERS or boxes.shape != (nm, 5, 2) or thr.shape != (nm, capi.MW_SAMPLE_CLASSES) or len(above) != nm:
        endrun("member_sample_mask_domain: 1 to %d members, and a (5, 2) box, an `above` bit and three thresholds for each, expected"
               % capi.MW_DOMAIN_MAX_MEMBERS)
    if counts is None:
        counts = torch.empty((nm, capi.MW_SAMPLE_WORDS), dtype=torch.int64, device=dev)
    if tuple(counts.shape) != (nm, capi.MW_SAMPLE_WORDS) or counts.dtype != torch.int64 or not counts.is_contiguous() or counts.device != dev:
        endrun("member_sample_mask_domain: counts must be a contiguous int64 tensor (%d, %d) on the fields' device" % (nm, capi.MW_SAMPLE_WORDS))
    if mask is not None and (mask.dtype != torch.uint8 or mask.numel() != f.numel() or not mask.is_contiguous() or mask.device != dev):
        endrun("member_sample_mask_domain: mask must be a contiguous uint8 tensor with one byte per element on the fields' device")
    with torch.cuda.device(dev):
        check(capi.lib().mw_member_sample_mask_domain(int(nz), n // int(nz), nens, nm, (C.c_int * nm)(*members),
                                                      boxes.ctypes.data_as(C.POINTER(C.c_double)), (C.c_int * nm)(*[int(bool(a)) for a in above]),
                                                      _field_ptr_array(list(fields5)), _field_ptr_array(list(teacher4)), int(key0) % 2 ** 64,
                                                      thr.ctypes.data_as(C.POINTER(C.c_double)), None if mask is None else C.c_void_p(mask.data_ptr()),
                                                      C.c_void_p(counts.data_ptr()), _stream_ptr(dev)))
    return counts


def harvest_outside_report(cfg, names, boxes, taken, eligible):
    """The three blocks `harvest:` gains in surrogate_rollout.json with `outside` -- pure Python: outside (the checked share, margin and
    fields, and `boxes`: {member: {field: [lo, hi]}}), taken and eligible ({member: {class of SAMPLE_CLASSES: samples / cells}},
    cumulative over the harvest calls)."""
    return {"outside": dict(cfg, boxes={str(n): box_json(b) for n, b in zip(names, boxes)}),
            "taken": {str(n): {c: int(taken[n][c]) for c in SAMPLE_CLASSES} for n in names},
            "eligible": {str(n): {c: int(eligible[n][c]) for c in SAMPLE_CLASSES} for n in names}}


class RolloutHarvester:
    """Data aggregation for the rollout (no reference counterpart): while the candidate models run online as ensemble members, ask the
    teacher -- Kessler -- what it would have done to each model member's OWN state, and keep (state, label) samples of it in one file per
    member, `rollout_samples_<name>.nc`, with exactly DataGenerator's dimensions and variables (surrogate_train.read_samples takes them
    unchanged).  harvest() is teacher -> mask -> nonzero -> gather -> append; the coupler's state is read, never written."""

    def init(self, coupler, member_names, members, directory, samples_per_step=50, ratio_active=0.5, prior_active=0.4, seed=None,
             max_rainsplit=64, outside=None, boxes=None, above=None):
        """member_names / members: the harvested model members' names and ensemble indices.  samples_per_step, ratio_active: the wanted
        samples per call and member and the wanted share of active cells among them (DataGenerator's 50 and 0.5); prior_active: the share
        of active cells assumed when the thresholds are set (DataGenerator's 0.4); seed: call c draws with seed + c (default: the clock).
        outside: None, or a mapping {share, margin, fields} -- share in (0, 1] of samples_per_step is asked of the cells
        outside the member's training box (harvest_thresholds), margin and fields are domain_config's and describe how `boxes` were
        made: one (5, 2) box per harvested member (domain_box) and, in `above`, one bool per member (its model reads the level above).
        The harvester then keeps taken[name] and eligible[name] ({class of SAMPLE_CLASSES: count}, cumulative) and last_counts, the raw
        (live members, 6) array of the last call."""
        import time as _time
        self.member_names, self.members = [str(n) for n in member_names], [int(m) for m in members]
        if len(self.member_names) != len(self.members) or not self.members or len(set(self.members)) != len(self.members) or \
                len(set(self.member_names)) != len(self.members):
            endrun("RolloutHarvester: as many distinct names as distinct members, at least one")
        if any(not 0 <= m < coupler.get_nens() for m in self.members):
            endrun("RolloutHarvester: members %r outside [0, %d)" % (self.members, coupler.get_nens()))
        if not (samples_per_step > 0 and 0.0 < ratio_active < 1.0 and 0.0 < prior_active < 1.0 and 1 <= int(max_rainsplit) <= 1024):
            endrun("RolloutHarvester: samples_per_step > 0, ratio_active and prior_active in (0, 1), max_rainsplit in [1, 1024]")
        self.samples_per_step, self.ratio_active, self.prior_active = float(samples_per_step), float(ratio_active), float(prior_active)
        self.max_rainsplit = int(max_rainsplit)
        self.seed = int(_time.time()) if seed is None else int(seed)
        self.files = {n: os.path.join(directory, "rollout_samples_%s.nc" % n) for n in self.member_names}
        for f in self.files.values():
            sample_file_create(f)
        self.samples = {n: 0 for n in self.member_names}
        self.skipped = {n: 0 for n in self.member_names}
        self.calls = 0
        self._meta_written = False
        self._teacher = None
        self.last_elems = None
        self.outside = self.boxes = self.above = self.last_counts = None
        if outside is not None:
            share = outside.get("share") if hasattr(outside, "get") else None
            if not hasattr(outside, "keys") or set(outside.keys()) != {"share", "margin", "fields"} or isinstance(share, bool) or \
                    not isinstance(share, (int, float)) or not 0.0 < share <= 1.0:
                endrun("RolloutHarvester: outside is None or a mapping {share in (0, 1], margin, fields}")
            self.outside = dict(share=float(share), **domain_config({k: outside[k] for k in ("margin", "fields")}, "RolloutHarvester: outside"))
            nm = len(self.members)
            if boxes is None or above is None or np.shape(boxes) != (nm, 5, 2) or len(above) != nm or nm > capi.MW_DOMAIN_MAX_MEMBERS:
                endrun("RolloutHarvester: outside needs one (5, 2) box and one `above` bit per harvested member, at most %d members"
                       % capi.MW_DOMAIN_MAX_MEMBERS)
            self.boxes, self.above = np.ascontiguousarray(boxes, dtype=np.float64), [bool(a) for a in above]
            self.taken = {n: {c: 0 for c in SAMPLE_CLASSES} for n in self.member_names}
            self.eligible = {n: {c: 0 for c in SAMPLE_CLASSES} for n in self.member_names}
        elif boxes is not None or above is not None:
            endrun("RolloutHarvester: boxes and above go with outside")

    def thresholds(self, coupler):
        """DataGenerator's two formulas (generate_micro_surrogate_data.h:58-62) per member, clamped to 1."""
        thr_act, thr_inact = sample_thresholds(self.ratio_active * self.samples_per_step, (1 - self.ratio_active) * self.samples_per_step,
                                               self.prior_active, coupler.get_nz() * coupler.get_ny() * coupler.get_nx())
        return min(1.0, thr_act), min(1.0, thr_inact)

    def _mask_outside(self, nz, ncol, f5, teacher, live, key0, mask):
        """The mask of a harvest with `outside`, in two calls of mw_member_sample_mask_domain on the live members: a count-only one, whose
        eligible-outside words -- this call's one extra synchronising host read -- fix each member's thresholds (harvest_thresholds), then
        the mask call with them.  self.last_thresholds: (live members, 3); self._counts: the mask call's device counts."""
        at = [self.member_names.index(n) for n, _ in live]
        members, boxes, above = [m for _, m in live], self.boxes[at], [self.above[j] for j in at]
        self._counts = member_sample_mask_domain(nz, f5, teacher, members, boxes, above, key0, np.zeros((len(live), 3)))
        outside = self._counts.cpu().numpy()[:, 0].tolist()
        self.last_thresholds = np.array([harvest_thresholds(self.samples_per_step, self.ratio_active, self.prior_active, nz * ncol,
                                                            self.outside["share"], int(q)) for q in outside], dtype=np.float64).reshape(len(live), 3)
        member_sample_mask_domain(nz, f5, teacher, members, boxes, above, key0, self.last_thresholds, mask, self._counts)

    def harvest(self, coupler, dt, etime):
        """One call: {name: samples added}.  A member the teacher skipped adds none and counts in `skipped`."""
        dm = coupler.get_data_manager_readonly()
        f5 = [dm.get(n, True) for n in ROLLOUT_IN5]
        nz, nens = coupler.get_nz(), coupler.get_nens()
        ncol = coupler.get_ny() * coupler.get_nx()
        nelem = nz * ncol * nens
        dev = coupler.device
        if self._teacher is None or self._teacher[0].shape != f5[0].shape:
            self._teacher = [torch.empty_like(f5[0]) for _ in range(4)]
        teacher, rs = kessler_members_teacher(coupler, self.members, dt, self.max_rainsplit, self._teacher, return_rainsplit=True)
        live = [(n, m) for n, m, r in zip(self.member_names, self.members, rs) if r > 0]
        for n, r in zip(self.member_names, rs):
            self.skipped[n] += int(r == 0)
        thr_act, thr_inact = self.thresholds(coupler)
        max_mag = (2 ** 64 - 1) // (1 + nelem)
        key0 = (((self.seed + self.calls) % max_mag) * nelem) % (2 ** 64)
        self.calls += 1
        added = {n: 0 for n in self.member_names}
        write_meta, self._meta_written = not self._meta_written, True
        ins = outs = which = None
        if live:
            L = capi.lib()
            mask = torch.empty(nelem, dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                if self.outside is None:
                    check(L.mw_member_sample_mask(nz, ncol, nens, len(live), (C.c_int * len(live))(*[m for _, m in live]), _field_ptr_array(f5),
                                                  _field_ptr_array(teacher), key0, thr_act, thr_inact, C.c_void_p(mask.data_ptr()), _stream_ptr(dev)))
                else:
                    self._mask_outside(nz, ncol, f5, teacher, live, key0, mask)
                elems, n, ins, outs = sample_buffers(mask)                     # ascending, as DataGenerator compacts
                check(L.mw_member_gather_samples(nz, ncol, nens, _field_ptr_array(f5), _field_ptr_array(teacher), C.c_void_p(elems.data_ptr()), n,
                                                 C.c_void_p(ins.data_ptr()), C.c_void_p(outs.data_ptr()), _stream_ptr(dev)))
            self.last_elems = elems.cpu().numpy()                              # (k * ncol + col) * nens + member of the samples (diagnostic)
            ins, outs, which = ins.cpu().numpy(), outs.cpu().numpy(), self.last_elems % nens
            if self.outside is not None:                                       # (the stream has been waited for: 48 bytes per member more)
                self.last_counts = self._counts.cpu().numpy().copy()
                for (name, _), row in zip(live, self.last_counts):
                    for c, cname in enumerate(SAMPLE_CLASSES):
                        self.eligible[name][cname] += int(row[c])
                        self.taken[name][cname] += int(row[capi.MW_SAMPLE_CLASSES + c])
        else:
            self.last_elems = np.zeros(0, dtype=np.int64)
            if self.outside is not None:
                self.last_counts = np.zeros((0, capi.MW_SAMPLE_WORDS), dtype=np.int64)
        for name, m in zip(self.member_names, self.members):
            sel = (which == m) if which is not None else np.zeros(0, dtype=bool)
            a = ins[sel] if which is not None else np.zeros((0, 5, 2), dtype=np.float32)
            b = outs[sel] if which is not None else np.zeros((0, 4), dtype=np.float32)
            sample_file_append(self.files[name], coupler, dt, a, b, write_meta)
            added[name] = int(a.shape[0])
            self.samples[name] += added[name]
        return added


def member_divergence(coupler, names):
    """mw_member_divergence of the coupler's fields `names` (at most 16, each (..., nens)): the raw arrays (stats, nonfinite) --
    stats (nens, len(names), 7) fp64 in the order of ROLLOUT_STATS (d = member - member 0 for the first four, the member's own values for
    the last three), nonfinite (nens, len(names)) int64, the member's NaN or inf elements -- from one device-to-host copy."""
    dm = coupler.get_data_manager_readonly()
    return fields_divergence(coupler, [dm.get(n, True) for n in names])


def fields_divergence(coupler, fields):
    """member_divergence of tensors (each (..., nens), one size) that need not be the coupler's own, such as a microphysics' rain_total."""
    nens = coupler.get_nens()
    n = fields[0].numel() // nens
    if any(t.numel() != n * nens or t.shape[-1] != nens for t in fields):
        endrun("member_divergence: the fields must have one size and the members last")
    L = capi.lib()
    nf = len(fields)
    nbytes = L.mw_member_divergence_workspace_bytes(n, nens, nf)
    if nbytes <= 0:
        endrun("member_divergence: %d fields of %d cells x %d members are out of range (at most %d fields)" % (nf, n, nens, capi.MW_MAX_TRACERS))
    ws = grown_workspace(coupler, "_ws_divergence", nbytes, coupler.device)
    buf = StatsAndCounts(nens * nf * 7, nens * nf, coupler.device)
    with torch.cuda.device(coupler.device):
        check(L.mw_member_divergence(n, nens, nf, _field_ptr_array(fields), _ptr(ws), buf.stats_ptr, buf.counts_ptr, _stream_ptr(coupler.device)))
    stats, nonfinite = buf.host()
    return stats.reshape(nens, nf, 7), nonfinite.reshape(nens, nf)


def rollout_report(stats, nonfinite, ncells, member_names, fields, cell_volume=1.0, persistence=None):
    """One scoring time's raw arrays (member_divergence) as a report -- pure numpy.  Per member and field: bias = sum d / n, mae, rmse and
    max_abs of d = member - Kessler member, rmse_over_persistence (None without a persistence member `persistence`, or when its rmse is
    0), the member's own mean, min, max and its count of non-finite elements.  A statistic that is inf or NaN is None and the field
    carries "finite": False.  Per member: total_water = cell_volume * sum of the three water fields (None unless all three are scored
    and finite) and finite = no field has a non-finite element or statistic."""
    stats = np.asarray(stats, dtype=np.float64)
    nonfinite = np.asarray(nonfinite, dtype=np.int64)
    if stats.shape != (len(member_names), len(fields), 7) or nonfinite.shape != stats.shape[:2]:
        endrun("rollout_report: stats must be (%d members, %d fields, 7) and nonfinite (%d, %d)" % ((len(member_names), len(fields)) * 2))
    n = float(ncells)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rmse = np.sqrt(stats[..., 2] / n)
        skill = rmse / rmse[persistence] if persistence is not None else None
    rep = {}
    for m, mname in enumerate(member_names):
        row, ok_member = {}, True
        for f, fname in enumerate(fields):
            q = None
            if persistence is not None and rmse[persistence, f] > 0:
                q = float(skill[m, f])
            row[fname] = finite_or_none({"bias": float(stats[m, f, 0] / n), "mae": float(stats[m, f, 1] / n), "rmse": float(rmse[m, f]),
                                         "max_abs": float(stats[m, f, 3]), "rmse_over_persistence": q, "mean": float(stats[m, f, 4] / n),
                                         "min": float(stats[m, f, 5]), "max": float(stats[m, f, 6]), "nonfinite": int(nonfinite[m, f])},
                                        bad=nonfinite[m, f] != 0)
            ok_member = ok_member and "finite" not in row[fname]
        water = None
        if all(w in fields for w in ROLLOUT_WATER):
            water = float(sum(stats[m, list(fields).index(w), 4] for w in ROLLOUT_WATER) * cell_volume)
            water = water if np.isfinite(water) else None
        rep[mname] = {"fields": row, "total_water": water, "finite": ok_member}
    return rep


class RolloutScorer:
    """Online skill of a rollout's members: accumulate(coupler, step, etime) at every scoring time, report() / table() at the end.
    member_names: rollout_member_names' list (a last member called persistence is the skill's denominator); fields: the coupler fields
    to score."""

    def __init__(self, member_names, fields=ROLLOUT_FIELDS):
        self.member_names = [str(m) for m in member_names]
        self.fields = [str(f) for f in fields]
        self.persistence = len(self.member_names) - 1 if self.member_names[-1] == "persistence" else None
        self.history = []               # per scoring time: step, etime, the raw arrays
        self.times = []                 # per scoring time: step, etime, rollout_report
        self.diverged_at = {m: None for m in self.member_names}

    def add(self, stats, nonfinite, ncells, cell_volume, step, etime):
        """One scoring time from raw arrays (what accumulate does after member_divergence): pure numpy."""
        rep = rollout_report(stats, nonfinite, ncells, self.member_names, self.fields, cell_volume, self.persistence)
        self.history.append({"step": int(step), "etime": float(etime), "stats": json_safe(np.asarray(stats, dtype=np.float64).tolist()),
                             "nonfinite": np.asarray(nonfinite).tolist()})
        self.times.append({"step": int(step), "etime": float(etime), "members": rep})
        for m in self.member_names:
            if self.diverged_at[m] is None and not rep[m]["finite"]:
                self.diverged_at[m] = {"step": int(step), "etime": float(etime)}
        return rep

    def accumulate(self, coupler, step, etime):
        stats, nonfinite = member_divergence(coupler, self.fields)
        ncells = coupler.get_nz() * coupler.get_ny() * coupler.get_nx()
        return self.add(stats, nonfinite, ncells, coupler.get_dx() * coupler.get_dy() * coupler.get_dz(), step, etime)

    def report(self):
        """{"times": one rollout_report per scoring time with its step and etime, "diverged_at": per member the first scoring time at
        which it showed a non-finite value, or None}."""
        if not self.times:
            endrun("RolloutScorer.report: nothing accumulated")
        return {"times": self.times, "diverged_at": dict(self.diverged_at)}

    def table(self, rep=None):
        """The last scoring time as text: one line per member, rmse against the Kessler member (/ persistence rmse) per field."""
        rep = self.report() if rep is None else rep
        last = rep["times"][-1]
        w = max(len(m) for m in self.member_names)
        lines = ["step %d, etime %.6f s" % (last["step"], last["etime"]),
                 "%-*s " % (w, "member") + " ".join("%26s" % ("%s rmse (/pers.)" % f) for f in self.fields) + "  diverged_at"]
        for m in self.member_names:
            row = last["members"][m]["fields"]
            cells = [skill_cell(row[f]["rmse"], row[f]["rmse_over_persistence"]) for f in self.fields]
            d = rep["diverged_at"][m]
            lines.append("%-*s " % (w, m) + " ".join(cells) + "  " + ("-" if d is None else "step %d" % d["step"]))
        return "\n".join(lines)


# ---- surface rain of every member from its column water budget -----------------------------------------------------------
RAIN_COUNTS = ("hits", "misses", "false_alarms", "correct_negatives", "nonfinite")
RAIN_FIELDS = ("rate_mm_h", "accumulation_mm")             # precl and rain_total in a report's units
RAIN_UNITS = (3.6e6, 1.0e3)                                # m of water / s -> mm / h, m -> mm
RAIN_DEFAULT_THRESHOLDS = (0.1, 1.0, 5.0, 10.0, 25.0)


def _water3(coupler):
    dm = coupler.get_data_manager_readonly()
    return [dm.get(n, True) for n in ROLLOUT_WATER]


def member_column_water(coupler, out=None):
    """mw_member_column_water of the coupler's three water tracers: the (ny, nx, nens) tensor of every member's column water,
    dz * sum over the levels of ((water_vapor + cloud_liquid) + precip_liquid), kg / m^2 (into `out`, of that shape, if given)."""
    ny, nx, nens = coupler.get_ny(), coupler.get_nx(), coupler.get_nens()
    if out is not None and (tuple(out.shape) != (ny, nx, nens) or not out.is_contiguous()):
        endrun("member_column_water: out must be a contiguous (ny, nx, nens) tensor")
    w = column_water(_water3(coupler), coupler.get_nz(), ny * nx, nens, coupler.get_dz(), None if out is None else out.view(-1))
    return w.view(ny, nx, nens)


def member_surface_rain(coupler, members, accum, dt, w_before, rain_total=None):
    """mw_member_surface_rain on the coupler's state and its `precl`: for the members in `members` (indices), precl becomes
    (w_before - member_column_water now) / (1000 dt), m of water / s, signed; then rain_total ((ny, nx, nens), metres; needed only with a
    non-empty `accum`) of the members in `accum` grows by dt * precl.  w_before: member_column_water before the step."""
    ny, nx, nens = coupler.get_ny(), coupler.get_nx(), coupler.get_nens()
    for t, what in ((w_before, "w_before"), (rain_total, "rain_total")):
        if t is not None and tuple(t.shape) != (ny, nx, nens):
            endrun("member_surface_rain: %s must be a (ny, nx, nens) tensor" % what)
    precl = coupler.get_data_manager_readwrite().get("precl")
    surface_rain_finish(_water3(coupler), coupler.get_nz(), ny * nx, nens, members, accum, coupler.get_dz(), dt, w_before, precl, rain_total)


def member_water_fix(coupler, members, accum, fixed, dt, w_before, rain_total=None, tolerance=0.0, excess=None):
    """mw_member_water_fix on the coupler's state and its `precl`: member_surface_rain that also acts.  A column of a member in `fixed`
    (indices, a subset of `members`) that holds more water than w_before by more than tolerance * w_before has water_vapor, cloud_liquid
    and precip_liquid scaled by w_before / (its water now); its precl is the budget of the state left behind.  temp and density_dry are
    never touched.  excess: None or a (ny, nx, nens) tensor that receives the water removed per column, kg / m^2.  Returns (counts
    (nens, 2) int64 = fixed, skipped columns; stats (nens, 2) fp64 = sum, max of the excess) as numpy arrays."""
    ny, nx, nens = coupler.get_ny(), coupler.get_nx(), coupler.get_nens()
    for t, what in ((w_before, "w_before"), (rain_total, "rain_total"), (excess, "excess")):
        if t is not None and (tuple(t.shape) != (ny, nx, nens) or not t.is_contiguous()):
            endrun("member_water_fix: %s must be a (ny, nx, nens) tensor" % what)
    precl = coupler.get_data_manager_readwrite().get("precl")
    out = water_fix_finish(_water3(coupler), coupler.get_nz(), ny * nx, nens, members, accum, fixed, tolerance, coupler.get_dz(), dt, w_before,
                           precl, rain_total, holder=coupler, excess=excess)
    stats, counts = out.host()
    return counts.reshape(nens, 2), stats.reshape(nens, 2)


def member_heat_closure(coupler, members, closed, dt, before2, tolerance=0.0, heating=None):
    """mw_member_heat_closure on the coupler's state.  before2: (temp_before, rho_v_before), two (nz, ny, nx, nens)
    tensors read at the elements of the members in `members` (indices).  Per cell of such a member r = temp - (temp_before + (lv / cp_d) *
    (rho_v_before - water_vapor) / density_dry); a cell of a member in `closed` (a subset of `members`) with |r| > tolerance gets the
    diagnosed temp; a cell with a non-finite r is skipped.  Only temp is written.  heating: None or a (ny, nx, nens) tensor that receives
    every column's spurious heating, W / m^2.  Returns (counts (nens, 2) int64 = closed, skipped cells; stats (nens, 6) fp64 = sum r,
    sum |r|, sum r^2, max |r|, sum H, max |H|, of the residual before closing) as numpy arrays."""
    nz, ny, nx, nens = coupler.get_nz(), coupler.get_ny(), coupler.get_nx(), coupler.get_nens()
    if len(before2) != 2 or any(tuple(t.shape) != (nz, ny, nx, nens) or not t.is_contiguous() for t in before2):
        endrun("member_heat_closure: before2 must be two (nz, ny, nx, nens) tensors")
    if heating is not None and (tuple(heating.shape) != (ny, nx, nens) or not heating.is_contiguous()):
        endrun("member_heat_closure: heating must be a (ny, nx, nens) tensor")
    dm = coupler.get_data_manager_readwrite()
    out = heat_closure_finish(dm.get("temp"), dm.get("density_dry", readonly=True), dm.get("water_vapor", readonly=True), before2, nz, ny * nx,
                              nens, members, closed, tolerance, coupler.get_dz(), dt, holder=coupler, heating=heating)
    stats, counts = out.host()
    return counts.reshape(nens, 2), stats.reshape(nens, 6)


def member_rain_table(coupler, fields, thresholds):
    """mw_member_rain_table of 1 .. 4 tensors (..., nens) of one size (such as precl and a rain_total) against member 0: per field an
    int64 array (its thresholds, nens, 5) in the order of RAIN_COUNTS.  thresholds: per field 1 .. 8 finite, strictly ascending numbers
    in the field's own unit; an event is x >= threshold.  One device-to-host copy."""
    nens, nf, cap = coupler.get_nens(), len(fields), capi.MW_RAIN_MAX_THRESHOLDS
    thresholds = [[float(x) for x in row] for row in thresholds]
    if not 1 <= nf <= capi.MW_RAIN_MAX_FIELDS or len(thresholds) != nf or any(not 1 <= len(row) <= cap for row in thresholds):
        endrun("member_rain_table: 1 to %d fields, each with 1 to %d thresholds of its own" % (capi.MW_RAIN_MAX_FIELDS, cap))
    ncol = fields[0].numel() // nens
    if any(t.numel() != ncol * nens or t.shape[-1] != nens for t in fields):
        endrun("member_rain_table: the fields must have one size and the members last")
    L = capi.lib()
    nbytes = L.mw_member_rain_table_workspace_bytes(ncol, nens, nf)
    if nbytes <= 0:
        endrun("member_rain_table: %d fields of %d columns x %d members are out of range (at most 64 members)" % (nf, ncol, nens))
    ws = grown_workspace(coupler, "_ws_rain_table", nbytes, coupler.device)
    buf = StatsAndCounts(0, nf * cap * nens * len(RAIN_COUNTS), coupler.device)
    thr = (C.c_double * (nf * cap))(*[row[j] if j < len(row) else 0.0 for row in thresholds for j in range(cap)])
    with torch.cuda.device(coupler.device):
        check(L.mw_member_rain_table(ncol, nens, nf, _field_ptr_array(fields), (C.c_int * nf)(*[len(row) for row in thresholds]), thr, _ptr(ws),
                                     buf.counts_ptr, _stream_ptr(coupler.device)))
    counts = buf.host()[1].reshape(nf, cap, nens, len(RAIN_COUNTS))
    return [counts[f, :len(row)].copy() for f, row in enumerate(thresholds)]


def rain_thresholds(values, what):
    """A checked threshold list of a surface_rain configuration: 1 .. 8 positive finite numbers, strictly ascending (ValueError)."""
    if not isinstance(values, (list, tuple)) or not 1 <= len(values) <= capi.MW_RAIN_MAX_THRESHOLDS:
        raise ValueError("ERROR: %s must be a list of 1 to %d numbers" % (what, capi.MW_RAIN_MAX_THRESHOLDS))
    if any(isinstance(x, bool) or not isinstance(x, (int, float)) or not np.isfinite(x) or not x > 0 for x in values):
        raise ValueError("ERROR: %s must hold positive finite numbers" % what)
    out = [float(x) for x in values]
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError("ERROR: %s must be strictly ascending" % what)
    return out


def _ratio(num, den):
    return None if den == 0 else float(num) / float(den)


def rain_scores(counts):
    """One threshold's five counts (RAIN_COUNTS' order) as a report row: the counts and csi = h / (h + m + f), pod = h / (h + m),
    far = f / (h + f), frequency_bias = (h + f) / (h + m), each None where its denominator is 0.  Pure Python."""
    h, m, f, cn, bad = (int(x) for x in counts)
    return {"hits": h, "misses": m, "false_alarms": f, "correct_negatives": cn, "nonfinite": bad, "csi": _ratio(h, h + m + f),
            "pod": _ratio(h, h + m), "far": _ratio(f, h + f), "frequency_bias": _ratio(h + f, h + m)}


def rain_report(stats, nonfinite, tables, ncol, member_names, thresholds_mm_h, thresholds_mm):
    """One scoring time's raw arrays as a report -- pure numpy.  stats (members, 2, 7) / nonfinite (members, 2): member_divergence's arrays
    of precl (m / s) and rain_total (m); tables: member_rain_table's two arrays.  Per member, RAIN_FIELDS' two blocks -- the rate in
    mm / h and the accumulation in mm: bias, mae, rmse and max_abs of d = member - Kessler member, the member's own mean, min, max, its
    count of non-finite columns (a statistic that is inf or NaN is None, and the block carries "finite": False), and `thresholds`: per
    threshold (in the block's unit) rain_scores' row."""
    stats = np.asarray(stats, dtype=np.float64)
    nonfinite = np.asarray(nonfinite, dtype=np.int64)
    thresholds = ([float(x) for x in thresholds_mm_h], [float(x) for x in thresholds_mm])
    tables = [np.asarray(t, dtype=np.int64) for t in tables]
    nm = len(member_names)
    if stats.shape != (nm, 2, 7) or nonfinite.shape != (nm, 2) or len(tables) != 2 or \
            any(t.shape != (len(thr), nm, len(RAIN_COUNTS)) for t, thr in zip(tables, thresholds)):
        endrun("rain_report: stats must be (%d members, 2, 7), nonfinite (%d, 2) and the tables (thresholds, %d, 5)" % (nm, nm, nm))
    n = float(ncol)
    rep = {}
    for m, mname in enumerate(member_names):
        rep[mname] = {}
        for f, (fname, unit) in enumerate(zip(RAIN_FIELDS, RAIN_UNITS)):
            s = stats[m, f]
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                row = {"bias": float(unit * (s[0] / n)), "mae": float(unit * (s[1] / n)), "rmse": float(unit * np.sqrt(s[2] / n)),
                       "max_abs": float(unit * s[3]), "mean": float(unit * (s[4] / n)), "min": float(unit * s[5]), "max": float(unit * s[6]),
                       "nonfinite": int(nonfinite[m, f])}
            row = finite_or_none(row, bad=nonfinite[m, f] != 0)
            row["thresholds"] = [dict(threshold=thr, **rain_scores(tables[f][j, m])) for j, thr in enumerate(thresholds[f])]
            rep[mname][fname] = row
    return rep


class RainScorer:
    """Every rollout member's surface rain against the Kessler member's: accumulate(coupler, micro, step, etime) at every scoring time,
    report() / table() at the end.  member_names: rollout_member_names' list; thresholds_mm_h / thresholds_mm: the events of the rate
    (precl, mm / h) and of the accumulation (micro.rain_total, mm), each 1 .. 8 positive, strictly ascending numbers."""

    def __init__(self, member_names, thresholds_mm_h=RAIN_DEFAULT_THRESHOLDS, thresholds_mm=RAIN_DEFAULT_THRESHOLDS):
        self.member_names = [str(m) for m in member_names]
        self.thresholds_mm_h = rain_thresholds(list(thresholds_mm_h), "thresholds_mm_h")
        self.thresholds_mm = rain_thresholds(list(thresholds_mm), "thresholds_mm")
        self.times = []                 # per scoring time: step, etime, rain_report

    def add(self, stats, nonfinite, tables, ncol, step, etime):
        """One scoring time from raw arrays (what accumulate does after the kernels): pure numpy."""
        rep = rain_report(stats, nonfinite, tables, ncol, self.member_names, self.thresholds_mm_h, self.thresholds_mm)
        self.times.append({"step": int(step), "etime": float(etime), "members": rep})
        return rep

    def accumulate(self, coupler, micro, step, etime):
        if getattr(micro, "rain_total", None) is None:
            endrun("RainScorer.accumulate: the microphysics holds no rain_total (Microphysics_Rollout.surface_rain is off, or no step ran)")
        fields = [coupler.get_data_manager_readonly().get("precl", True), micro.rain_total]
        stats, nonfinite = fields_divergence(coupler, fields)
        tables = member_rain_table(coupler, fields, [[x / RAIN_UNITS[0] for x in self.thresholds_mm_h],
                                                     [x / RAIN_UNITS[1] for x in self.thresholds_mm]])
        return self.add(stats, nonfinite, tables, coupler.get_ny() * coupler.get_nx(), step, etime)

    def report(self):
        """{"thresholds_mm_h", "thresholds_mm", "times": one rain_report per scoring time with its step and etime}."""
        if not self.times:
            endrun("RainScorer.report: nothing accumulated")
        return {"thresholds_mm_h": list(self.thresholds_mm_h), "thresholds_mm": list(self.thresholds_mm), "times": self.times}

    def table(self, rep=None):
        """The last scoring time as text, one line per member: mean and rmse (against the Kessler member) of the rate and of the
        accumulation, and the accumulation's critical success index at its lowest threshold."""
        rep = self.report() if rep is None else rep
        last = rep["times"][-1]
        w = max(len(m) for m in self.member_names)
        lines = ["surface rain at step %d, etime %.6f s" % (last["step"], last["etime"]),
                 "%-*s %14s %14s %14s %14s %12s" % (w, "member", "rate mm/h", "rmse", "total mm", "rmse", "csi>=%gmm" % rep["thresholds_mm"][0])]
        for m in self.member_names:
            r, a = last["members"][m]["rate_mm_h"], last["members"][m]["accumulation_mm"]
            lines.append("%-*s %14s %14s %14s %14s %12s" % (w, m, or_dash(r["mean"], "%.6e"), or_dash(r["rmse"], "%.6e"), or_dash(a["mean"], "%.6e"),
                                                            or_dash(a["rmse"], "%.6e"), or_dash(a["thresholds"][0]["csi"], "%.4f")))
        return "\n".join(lines)
