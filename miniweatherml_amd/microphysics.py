"""The microphysics in charge of a run, thin drivers of mw_kessler_time_step and of the surrogate's forward passes:

  Microphysics_Kessler               model/modules/microphysics_kessler.h:8-346
  Microphysics_Kessler_Surrogate     experiments/supercell_kessler_surrogate/custom_modules/microphysics_kessler_ponni.h:149-278

No arithmetic happens in Python: everything runs in libmw_cdna4.so on the GPU (no fallback)."""
import ctypes as C
import types

import torch

from . import capi
from ._ffi import StatsAndCounts, _field_ptr_array, _ptr, _stream_ptr, grown_workspace
from .capi import check
from .coupler import endrun
from .mlp import OUT4, as_surrogate_model, load_surrogate_model, mlp_forward, mlp_stencil_forward
from .surrogate_eval import SurrogateBank


def column_water(water3, nz, ncol, nens, dz, out=None):
    """mw_member_column_water of three member-fastest (nz, ncol, nens) tensors (water_vapor, cloud_liquid, precip_liquid): the
    (ncol * nens,) tensor of dz * sum_k ((rho_v + rho_c) + rho_r), kg / m^2, written into `out` if given."""
    dev = water3[0].device
    if out is None:
        out = torch.empty(ncol * nens, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(capi.lib().mw_member_column_water(nz, ncol, nens, _field_ptr_array(water3), float(dz), _ptr(out), _stream_ptr(dev)))
    return out


def surface_rain_finish(water3, nz, ncol, nens, members, accum, dz, dt, w_before, precl, rain_total=None):
    """mw_member_surface_rain: precl of the members in `members` becomes (w_before - column water of water3 now) / (1000 dt), then
    rain_total of the members in `accum` grows by dt * precl.  Every other element keeps its bits."""
    dev = water3[0].device
    members, accum = [int(m) for m in members], [int(m) for m in accum]
    with torch.cuda.device(dev):
        check(capi.lib().mw_member_surface_rain(nz, ncol, nens, len(members), (C.c_int * max(1, len(members)))(*members), len(accum),
                                                (C.c_int * max(1, len(accum)))(*accum), _field_ptr_array(water3), float(dz), float(dt),
                                                _ptr(w_before) if w_before is not None else None, _ptr(precl),
                                                _ptr(rain_total) if rain_total is not None else None, _stream_ptr(dev)))


def water_fix_finish(water3, nz, ncol, nens, members, accum, fixed, tolerance, dz, dt, w_before, precl, rain_total=None, holder=None,
                     excess=None):
    """mw_member_water_fix: surface_rain_finish that also acts.  A column of a member in `fixed` (a subset of `members`)
    that holds more water than w_before, by more than tolerance * w_before, has its three water fields scaled back to w_before; its precl
    is the budget of the state left behind.  Every other element gets surface_rain_finish's bits.  Returns the StatsAndCounts of the
    call, on the device: 2 * nens doubles (sum and maximum of the excess per member, kg / m^2) and 2 * nens counts (fixed and skipped
    columns per member).  holder: the object that keeps the workspace and that buffer between calls; excess: an (ncol * nens) tensor."""
    dev = water3[0].device
    members, accum, fixed = [int(m) for m in members], [int(m) for m in accum], [int(m) for m in fixed]
    L = capi.lib()
    nbytes = L.mw_member_water_fix_workspace_bytes(ncol, nens)
    if nbytes <= 0:
        endrun("water_fix_finish: %d columns x %d members are out of range (at most 64 members)" % (ncol, nens))
    holder = holder if holder is not None else types.SimpleNamespace()
    ws = grown_workspace(holder, "_ws_water_fix", nbytes, dev)
    held = getattr(holder, "_water_fix_out", None)
    out = StatsAndCounts(2 * nens, 2 * nens, dev, held.buf if held is not None and held.buf.numel() == 4 * nens and held.buf.device == ws.device
                         else None)
    holder._water_fix_out = out
    ints = lambda v: (C.c_int * max(1, len(v)))(*v)                            # noqa: E731
    with torch.cuda.device(dev):
        check(L.mw_member_water_fix(nz, ncol, nens, len(members), ints(members), len(accum), ints(accum), len(fixed), ints(fixed),
                                    float(tolerance), _field_ptr_array(water3), float(dz), float(dt),
                                    _ptr(w_before) if w_before is not None else None, _ptr(precl),
                                    _ptr(rain_total) if rain_total is not None else None, _ptr(ws), out.counts_ptr, out.stats_ptr,
                                    _ptr(excess) if excess is not None else None, _stream_ptr(dev)))
    return out


LV, CP_D = 2.5e6, 1003.0       # Kessler's latent heat of vaporisation (microphysics_kessler.h:247) and cp_d (:32), the closure's constants


def members_copy(n, nens, members, src, dst):
    """mw_members_copy: the listed members' elements of the member-fastest (n, nens) tensors `src` into `dst` (1 .. 8 pairs)."""
    dev = src[0].device
    members = [int(m) for m in members]
    with torch.cuda.device(dev):
        check(capi.lib().mw_members_copy(n, nens, len(members), (C.c_int * max(1, len(members)))(*members), len(src), _field_ptr_array(src),
                                         _field_ptr_array(dst), _stream_ptr(dev)))


def heat_closure_finish(temp, rho_d, rho_v, before2, nz, ncol, nens, members, closed, tolerance, dz, dt, holder=None, heating=None,
                        lv=LV, cp_d=CP_D):
    """mw_member_heat_closure, its one caller.  Per cell of a member in `members`, T_c = temp_before + (lv / cp_d) *
    (rho_v_before - rho_v) / rho_d and r = temp - T_c; a cell of a member in `closed` (a subset of `members`) with |r| > tolerance gets
    temp = T_c; a cell whose r is not finite is skipped.  before2: (temp_before, rho_v_before), read at the diagnosed members' elements.
    Returns the StatsAndCounts of the call, on the device: 6 * nens doubles (sum r, sum |r|, sum r^2, max |r|, sum H, max |H| per member,
    of the residual BEFORE closing) and 2 * nens counts (closed and skipped cells per member).  holder: the object that keeps the workspace
    and that buffer between calls; heating: an (ncol * nens) tensor that receives every column's spurious heating H, W / m^2."""
    dev = temp.device
    members, closed = [int(m) for m in members], [int(m) for m in closed]
    L = capi.lib()
    nbytes = L.mw_member_heat_closure_workspace_bytes(ncol, nens)
    if nbytes <= 0:
        endrun("heat_closure_finish: %d columns x %d members are out of range (at most 64 members)" % (ncol, nens))
    holder = holder if holder is not None else types.SimpleNamespace()
    ws = grown_workspace(holder, "_ws_heat_closure", nbytes, dev)
    held = getattr(holder, "_heat_closure_out", None)
    out = StatsAndCounts(6 * nens, 2 * nens, dev, held.buf if held is not None and held.buf.numel() == 8 * nens and held.buf.device == ws.device
                         else None)
    holder._heat_closure_out = out
    ints = lambda v: (C.c_int * max(1, len(v)))(*v)                            # noqa: E731
    with torch.cuda.device(dev):
        check(L.mw_member_heat_closure(nz, ncol, nens, len(members), ints(members), len(closed), ints(closed), float(tolerance), float(lv),
                                       float(cp_d), float(dz), float(dt), _ptr(temp), _ptr(rho_d), _ptr(rho_v), _field_ptr_array(list(before2)),
                                       _ptr(ws), out.counts_ptr, out.stats_ptr, _ptr(heating) if heating is not None else None,
                                       _stream_ptr(dev)))
    return out


def water_fix_tolerance(value, what):
    """A checked tolerance of a water fixer: a finite number >= 0 (ValueError)."""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not (value >= 0.0 and value - value == 0.0):
        raise ValueError("ERROR: %s must be a finite number >= 0, not %r" % (what, value))
    return float(value)


class Microphysics_Kessler:
    num_tracers = 3
    ID_V, ID_C, ID_R = 0, 1, 2

    def __init__(self):                                                        # microphysics_kessler.h:29-41
        self.R_d, self.cp_d = 287., 1003.
        self.cv_d = self.cp_d - self.R_d
        self.gamma_d = self.cp_d / self.cv_d
        self.kappa_d = self.R_d / self.cp_d
        self.R_v, self.cp_v = 461., 1859.
        self.cv_v = self.R_v - self.cp_v
        self.p0, self.grav = 1.e5, 9.81
        self._ws = None
        self.strict = 0          # 1: the strict path (reference operation order, glibc's pow / exp): bit-identical to the CPU oracle

    def set_strict(self, strict):
        self.strict = int(bool(strict))

    @staticmethod
    def get_num_tracers():
        return 3

    def micro_name(self):
        return "kessler"

    def init(self, coupler):                                                   # :51-96
        coupler.add_tracer("water_vapor", "Water Vapor", True, True)
        coupler.add_tracer("cloud_liquid", "Cloud liquid", True, True)
        coupler.add_tracer("precip_liquid", "precip_liquid", True, True)
        dm = coupler.get_data_manager_readwrite()
        dm.register_and_allocate("precl", "precipitation rate", (coupler.get_ny(), coupler.get_nx(), coupler.get_nens()),
                                 ["y", "x", "nens"])
        coupler.set_option("micro", "kessler")
        for k in ("R_d", "cp_d", "cv_d", "gamma_d", "kappa_d", "R_v", "cp_v", "cv_v", "p0", "grav"):
            coupler.set_option(k, getattr(self, k))

    def time_step(self, coupler, dt, return_rainsplit=False):                  # :99-162
        dm = coupler.get_data_manager_readwrite()
        rho_v, rho_c, rho_r = dm.get("water_vapor"), dm.get("cloud_liquid"), dm.get("precip_liquid")
        rho_d, temp, precl = dm.get("density_dry", readonly=True), dm.get("temp"), dm.get("precl")
        nz = coupler.get_nz()
        ncol = coupler.get_ny() * coupler.get_nx() * coupler.get_nens()
        L = capi.lib()
        ws = grown_workspace(self, "_ws", L.mw_kessler_workspace_bytes(nz, ncol), coupler.device)
        rs = C.c_int(0)
        check(L.mw_kessler_set_strict(self.strict))
        with torch.cuda.device(coupler.device):
            check(L.mw_kessler_time_step(nz, ncol, coupler.get_dz(), float(dt), _ptr(rho_v), _ptr(rho_c), _ptr(rho_r), _ptr(rho_d),
                                         _ptr(temp), _ptr(precl), _ptr(ws), C.byref(rs) if return_rainsplit else None,
                                         _stream_ptr(coupler.device)))
        return rs.value if return_rainsplit else None


class Microphysics_Kessler_Surrogate(Microphysics_Kessler):
    """custom_modules::Microphysics_Kessler of the surrogate experiment: NN inference beside the true Kessler
    (microphysics_kessler_ponni.h:149-278).  The NN result is returned (and diffed) but not written back,
    exactly like the reference with lines :273-276 commented out.  With `online` the result replaces the state, and `precl` would still
    be Kessler's; `surface_rain = True` then makes it the column water budget of the state that stays."""

    online = False        # True = the four deep_copy_to lines :273-276 un-commented: the NN result replaces Kessler's
    mlp_strict = 0        # 1: the thread-per-cell MLP that accumulates in index order (bit-identical to the CPU restatement; tests)

    want_range = False    # with a committee: time_step also fills last_range, the four fields of the members' spread
    last_range = None
    surface_rain = False  # True (with online only): precl after the step is the column water budget of the state left in the coupler
    water_fixer = None    # True or {tolerance} (with online only): a column that gained water in the step is scaled back
    last_water_fix = None  # with water_fixer: the StatsAndCounts of the last step, on the device (water_fix_stats fetches it)
    heat_closure = None   # True or {tolerance} (with online only): temp becomes what the network's own vapour change makes it
    last_heat_closure = None  # with heat_closure: the StatsAndCounts of the last step, on the device (heat_closure_stats fetches it)

    def init(self, coupler, weights_txt=None, in_scaling_txt=None, out_scaling_txt=None, weights_h5=None, committee=None, guard=None,
             domains=None):
        """Single-model files: the model's output form is the one its output scaling file declares (self.form: "state" | "tendency";
        mlp.load_surrogate_model).  committee: a list of 1 .. 16 (W1, b1, W2, b2, scl_in, scl_out) tuples of one width (load_surrogate_weights'
        form, the state form) or SurrogateModel tuples with the form last; a committee may mix the forms.  The network's
        result is then the committee's mean (SurrogateBank.committee_apply), and the weight file arguments are not read.  guard
        (surrogate_eval.guard_config's mapping; with a committee only): the result is the GUARDED committee's step of the state before the
        call -- the mean, and on the columns where the models' range exceeds a threshold what Kessler leaves on those columns alone.  A
        guard with `domain` hands Kessler the columns with a cell outside the committee's training box too; domains: None, or
        per committee model None or its training-domain table (mlp.load_training_domain), which that box is then made of."""
        super().init(coupler)
        self._nn_out = None
        self._committee = None
        self._guard_cfg = self._guard = self._guard_box = None
        if guard is not None:
            if committee is None:
                endrun("Microphysics_Kessler_Surrogate: a guard needs a committee")
            from .surrogate_eval import guard_config
            self._guard_cfg = guard_config(guard, "the committee's guard")
        if committee is not None:
            committee = list(committee)
            if any(k is not None for k in (weights_txt, in_scaling_txt, out_scaling_txt, weights_h5)):
                endrun("Microphysics_Kessler_Surrogate: a committee brings its own weights and scaling tables: give no file beside it")
            if not 1 <= len(committee) <= capi.MW_COMMITTEE_MAX_MODELS:
                endrun("Microphysics_Kessler_Surrogate: a committee has 1 to %d models, got %d" % (capi.MW_COMMITTEE_MAX_MODELS, len(committee)))
            self._committee = SurrogateBank(committee, coupler.device)
            self.W1, self.b1, self.W2, self.b2, self.scl_in, self.scl_out, self.form = as_surrogate_model(committee[0])
            if self._guard_cfg is not None and "domain" in self._guard_cfg:
                from .surrogate_eval import domain_box
                self._guard_box = domain_box(committee, self._guard_cfg["domain"]["margin"], self._guard_cfg["domain"]["fields"],
                                             tables=domains)
            return
        self.W1, self.b1, self.W2, self.b2, self.scl_in, self.scl_out, self.form = load_surrogate_model(weights_txt, in_scaling_txt,
                                                                                                        out_scaling_txt, weights_h5)

    def time_step(self, coupler, dt):
        dm = coupler.get_data_manager_readwrite()
        temp, rho_d = dm.get("temp"), dm.get("density_dry", readonly=True)
        rho_v, rho_c, rho_r = dm.get("water_vapor"), dm.get("cloud_liquid"), dm.get("precip_liquid")
        if getattr(self, "_committee", None) is not None:
            guarded = getattr(self, "_guard_cfg", None) is not None            # (the guard's scratch holds the result and the range)
            if self._nn_out is None and not guarded:
                self._nn_out = [torch.empty_like(temp) for _ in range(4)]
            if self.want_range and self.last_range is None and not guarded:
                self.last_range = [torch.empty_like(temp) for _ in range(4)]
            self._committee.strict = self.mlp_strict
            # the coupler's fields are (nz, ny, nx, nens): every member is one more column, so the whole array is one member of nens = 1
            flat = [t.reshape(coupler.get_nz(), -1, 1) for t in (temp, rho_d, rho_v, rho_c, rho_r)]
            if guarded:
                from .surrogate_eval import CommitteeGuard
                g = self._guard_cfg
                if self._guard is None:
                    self._guard = CommitteeGuard(flat[0], coupler.get_nz())
                self._committee.committee_guard_flag(coupler.get_nz(), range(self._committee.models), 0, flat, [g[f] for f in OUT4], self._guard,
                                                     domain_box=getattr(self, "_guard_box", None))
                self._guard.commit(coupler.get_nz(), [0], flat, g["max_rainsplit"], coupler.get_dz(), dt, copy=False)   # Kessler below writes the state
                self._nn_out = [t.reshape(temp.shape) for t in self._guard.mean4]
                if self.want_range:
                    self.last_range = [t.reshape(temp.shape) for t in self._guard.range4]
                return self._finish_step(coupler, dt, temp, rho_v, rho_c, rho_r)
            self._committee.committee_apply(coupler.get_nz(), range(self._committee.models), 0, flat,
                                            [t.reshape(coupler.get_nz(), -1, 1) for t in self._nn_out],
                                            [t.reshape(coupler.get_nz(), -1, 1) for t in self.last_range] if self.want_range else None)
        elif self.W1.shape[0] == 9:                                            # the stencil model: what load_surrogate_model found
            self._nn_out = mlp_stencil_forward(coupler.get_nz(), temp, rho_d, rho_v, rho_c, rho_r, self.W1, self.b1, self.W2, self.b2,
                                               self.scl_in, self.scl_out, self._nn_out, strict=self.mlp_strict, form=getattr(self, "form", "state"))
        else:
            self._nn_out = mlp_forward(temp, rho_d, rho_v, rho_c, rho_r, self.W1, self.b1, self.W2, self.b2, self.scl_in, self.scl_out,
                                       self._nn_out, strict=self.mlp_strict, form=getattr(self, "form", "state"))
        return self._finish_step(coupler, dt, temp, rho_v, rho_c, rho_r)

    def _finish_step(self, coupler, dt, temp, rho_v, rho_c, rho_r):
        fixer = self._water_fixer_tolerance()
        budget = bool(self.surface_rain) or fixer is not None
        if budget:
            if fixer is not None and not self.online:
                endrun("Microphysics_Kessler_Surrogate: water_fixer needs online = True (offline the state is Kessler's, which makes no water)")
            if not self.online:
                endrun("Microphysics_Kessler_Surrogate: surface_rain needs online = True (offline the state is Kessler's, and so is precl)")
            # every member is one more column: the whole (ny * nx * nens) plane is one member's columns (the network's result is still
            # out of place, so this is the state before the call)
            nz, ncol = coupler.get_nz(), coupler.get_ny() * coupler.get_nx() * coupler.get_nens()
            held = getattr(self, "_w_before", None)
            self._w_before = column_water([rho_v, rho_c, rho_r], nz, ncol, 1, coupler.get_dz(),
                                          held if held is not None and held.numel() == ncol else None)
        closure = self._heat_closure_tolerance()
        if closure is not None:                                                # temp and water_vapor before the call: the plane is one member
            if not self.online:
                endrun("Microphysics_Kessler_Surrogate: heat_closure needs online = True (offline the state is Kessler's, which obeys the closure)")
            held = getattr(self, "_heat_before", None)
            if held is None or held[0].shape != temp.shape or held[0].device != temp.device:
                self._heat_before = held = [torch.empty_like(temp), torch.empty_like(temp)]
            members_copy(temp.numel(), 1, [0], [temp, rho_v], held)
        super().time_step(coupler, dt)
        if self.online:                                                        # :273-276
            self._diffs = self.mean_diffs(coupler)                             # (the prints of :266-269 come first)
            for dst, src in zip((temp, rho_v, rho_c, rho_r), self._nn_out):
                dst.copy_(src)
        if closure is not None:                                                # before the fixer: the vapour change is the network's
            rho_d = coupler.get_data_manager_readonly().get("density_dry", True)
            self.last_heat_closure = heat_closure_finish(temp, rho_d, rho_v, self._heat_before, coupler.get_nz(), temp.numel() // coupler.get_nz(),
                                                         1, [0], [0], closure, coupler.get_dz(), dt, holder=self)
        if budget:                                                             # Kessler's precl gives way to the budget of the state that stays
            precl = coupler.get_data_manager_readwrite().get("precl")
            if fixer is None:
                surface_rain_finish([rho_v, rho_c, rho_r], nz, ncol, 1, [0], [], coupler.get_dz(), dt, self._w_before, precl)
            else:                                                              # ... and a column that gained water gives it back
                self.last_water_fix = water_fix_finish([rho_v, rho_c, rho_r], nz, ncol, 1, [0], [], [0], fixer, coupler.get_dz(), dt,
                                                       self._w_before, precl, holder=self)
        return self._nn_out            # (temp_tmp, rho_v_tmp, rho_c_tmp, rho_r_tmp)

    def _water_fixer_tolerance(self):
        """None without `water_fixer`; else its checked tolerance."""
        wf = self.water_fixer
        if wf is None or wf is False:
            return None
        if wf is True:
            return 0.0
        if not hasattr(wf, "keys") or set(wf.keys()) - {"tolerance"}:
            endrun("Microphysics_Kessler_Surrogate: water_fixer is None, True or a mapping whose only key is tolerance")
        try:
            return water_fix_tolerance(wf.get("tolerance", 0.0), "water_fixer.tolerance")
        except ValueError as err:
            endrun("Microphysics_Kessler_Surrogate: " + str(err))

    def _heat_closure_tolerance(self):
        """None without `heat_closure`; else its checked tolerance."""
        hc = self.heat_closure
        if hc is None or hc is False:
            return None
        if hc is True:
            return 0.0
        if not hasattr(hc, "keys") or set(hc.keys()) - {"tolerance"}:
            endrun("Microphysics_Kessler_Surrogate: heat_closure is None, True or a mapping whose only key is tolerance")
        try:
            return water_fix_tolerance(hc.get("tolerance", 0.0), "heat_closure.tolerance")
        except ValueError as err:
            endrun("Microphysics_Kessler_Surrogate: " + str(err))

    def heat_closure_stats(self):
        """The last step's closure statistics of the whole plane, fetched from the device: cells_closed, cells_skipped, residual_K {sum,
        sum_abs, sum_sq, max}, heating_W_m2 {sum, max}; None before the first step with `heat_closure`."""
        if self.last_heat_closure is None:
            return None
        stats, counts = self.last_heat_closure.host()
        return {"cells_closed": int(counts[0]), "cells_skipped": int(counts[1]),
                "residual_K": {"sum": float(stats[0]), "sum_abs": float(stats[1]), "sum_sq": float(stats[2]), "max": float(stats[3])},
                "heating_W_m2": {"sum": float(stats[4]), "max": float(stats[5])}}

    def water_fix_stats(self):
        """The last step's fixer statistics of the whole plane, fetched from the device: columns_fixed, columns_skipped,
        water_removed_kg_m2 {sum, max}; None before the first step with `water_fixer`."""
        if self.last_water_fix is None:
            return None
        stats, counts = self.last_water_fix.host()
        return {"columns_fixed": int(counts[0]), "columns_skipped": int(counts[1]),
                "water_removed_kg_m2": {"sum": float(stats[0]), "max": float(stats[1])}}

    def mean_diffs(self, coupler):
        """The four 'Relative diff' prints (:266-269): mean(NN - Kessler)."""
        dm = coupler.get_data_manager_readonly()
        t, v, c, r = self._nn_out
        if getattr(self, "_ws_mean", None) is None:
            self._ws_mean = torch.empty(1024, dtype=torch.float64, device=coupler.device)
        out = {}
        with torch.cuda.device(coupler.device):
            for key, nn, name in (("rho_v", v, "water_vapor"), ("rho_c", c, "cloud_liquid"), ("rho_r", r, "precip_liquid"), ("temp", t, "temp")):
                m = C.c_double(0.0)
                check(capi.lib().mw_mean_diff(nn.numel(), _ptr(nn), _ptr(dm.get(name, True)), _ptr(self._ws_mean), C.byref(m),
                                              _stream_ptr(coupler.device)))
                out[key] = m.value
        return out
