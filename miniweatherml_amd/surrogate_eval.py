"""In-loop evaluation of candidate surrogate networks against the microphysics in charge (no reference counterpart; the networks are
those of experiments/supercell_kessler_surrogate/custom_modules/microphysics_kessler_ponni.h:97-202):

  SurrogateBank                        mw_surrogate_bank_t: K networks of one width on the device; evaluate, members_apply, committee_apply
  eval_domain_config, DomainSplitEvaluator   the evaluation split by inside / outside each model's training box (mw_surrogate_eval_domain)
  surrogate_scores, SurrogateEvaluator exact accumulation of mw_surrogate_eval's statistics, report and table
  committee_score, CommitteeEvaluator  mw_committee_score: the committee's mean and range against the truth
  json_safe, finite_or_none, skill_cell, the exact-sum helpers: pure numpy / Python, shared with the rollout's reports"""
import ctypes as C

import numpy as np
import torch

from . import capi
from ._ffi import StatsAndCounts, _field_ptr_array, _ptr, _stream_ptr, fit_workspace, grown_workspace
from .capi import check
from .coupler import endrun
from .mlp import FORMS, IN5, OUT4, as_surrogate_model, strict_mode

EVAL_FIELDS = OUT4
EVAL_CLASSES = ("inactive", "active")
_EXACT_ONE = 1 << 1074            # sums are kept as integers in units of 2^-1074, the spacing of the smallest doubles: exact addition


class SurrogateBank:
    """mw_surrogate_bank_t: K candidate networks of one width (all single-cell or all stencil), each with its own scaling tables, uploaded
    once to `device`; evaluate() refuses fields of another device.  models: a list of (W1, b1, W2, b2, scl_in, scl_out) as
    load_surrogate_weights returns them (the state form) or of SurrogateModel tuples with the form last (load_surrogate_model); a bank may
    hold both forms.  self.forms: the models' forms by name."""

    def __init__(self, models, device="cuda:0"):
        self._h = None
        self.device = torch.device(device)
        models = list(models)
        if len(models) < 1:
            endrun("SurrogateBank: no models")
        models = [as_surrogate_model(m) for m in models]
        self.forms = [m.form for m in models]
        if len(models) > capi.MW_SURROGATE_MAX_MODELS:
            endrun("SurrogateBank: %d models, at most %d fit one bank" % (len(models), capi.MW_SURROGATE_MAX_MODELS))
        widths = sorted({int(np.asarray(m[0]).shape[0]) for m in models})
        if len(widths) != 1:
            endrun("SurrogateBank: models of different widths (%s inputs) cannot share a bank: one bank per width" % ", ".join(map(str, widths)))
        self.n_in, self.models = widths[0], len(models)
        a = 10 * self.n_in
        for W1, b1, W2, b2, si, so, _ in models:
            if np.shape(W1) != (self.n_in, 10) or np.shape(b1) != (10,) or np.shape(W2) != (10, 4) or np.shape(b2) != (4,) or \
                    np.shape(si) != (self.n_in, 2) or np.shape(so) != (4, 2):
                endrun("SurrogateBank: a model is not Dense(%d->10), Dense(10->4) with (%d, 2) and (4, 2) scaling tables" % (self.n_in, self.n_in))
        params = np.ascontiguousarray([np.concatenate([np.ravel(m[0]), np.ravel(m[1]), np.ravel(m[2]), np.ravel(m[3])]) for m in models], dtype=np.float32)
        scl_in = np.ascontiguousarray([m[4] for m in models], dtype=np.float64)
        scl_out = np.ascontiguousarray([m[5] for m in models], dtype=np.float64)
        forms = (C.c_int * len(models))(*[FORMS.index(f) for f in self.forms])
        h = C.c_void_p()
        if capi.lib().mw_device_count() < 1:
            endrun("SurrogateBank: no HIP device available: libmw_cdna4 has no CPU fallback")
        with torch.cuda.device(self.device):                              # the handle's allocations live on the current device
            check(capi.lib().mw_surrogate_bank_create_forms(C.byref(h), self.n_in, self.models, params.ctypes.data_as(C.POINTER(C.c_float)),
                                                            scl_in.ctypes.data_as(C.POINTER(C.c_double)),
                                                            scl_out.ctypes.data_as(C.POINTER(C.c_double)), forms))
        self._h = h
        self.group = int(capi.lib().mw_surrogate_eval_group(h))           # models per pass over the state
        self.domain_group = int(capi.lib().mw_surrogate_eval_domain_group(h))   # ... whose predictions evaluate_domain scores per pass
        self.strict = 0                                                   # 1: the thread-per-cell kernels (mw_mlp_set_strict)
        self._buf = None
        self.boxes = None                                                 # set_domain's (K, 5, 2) boxes
        self._dbuf = None

    def __del__(self):
        try:                                                              # (at interpreter exit the module's globals may be gone)
            if getattr(self, "_h", None):
                with torch.cuda.device(self.device):
                    capi.lib().mw_surrogate_bank_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _eval_layout(self, who, nz, in5, truth4):
        """(cells, device) of evaluate's nine fields; refuses, in the caller's name `who`, a wrong number of fields, fields of different
        sizes or of no whole number of columns, and fields off the bank's device."""
        if len(in5) != 5 or len(truth4) != 4:
            endrun(who + "five input fields and four truth fields expected")
        n = in5[0].numel()
        if int(nz) < 1 or n % int(nz) != 0 or any(t.numel() != n for t in list(in5) + list(truth4)):
            endrun(who + "the nine fields must have one size, a whole number of columns of nz = %d levels" % nz)
        dev = self.device
        if any(t.device != dev for t in list(in5) + list(truth4)):
            endrun(who + "the bank lives on %s, the fields on %s" % (dev, sorted({str(t.device) for t in list(in5) + list(truth4)})))
        return n, dev

    def evaluate(self, nz, in5, truth4):
        """in5: the five fields before the microphysics call (temp, density_dry, water_vapor, cloud_liquid, precip_liquid), truth4: the four
        after it (EVAL_FIELDS); fp64 CUDA tensors of nz levels.  Returns (stats, counts): the raw (K + 1, 2, 4, 4) fp64 array
        [model | persistence][inactive, active][field][sum d, sum |d|, sum d^2, max |d|], d = prediction - truth, and the int64 cells per
        class -- one device-to-host copy for both."""
        n, dev = self._eval_layout("SurrogateBank.evaluate: ", nz, in5, truth4)
        buf = StatsAndCounts((self.models + 1) * 32, 2, dev, self._buf)
        self._buf = buf.buf                                               # (the int64 tensor itself: kept from call to call)
        with strict_mode(self.strict), torch.cuda.device(dev):
            rc = capi.lib().mw_surrogate_eval(self._h, int(nz), n // int(nz), _field_ptr_array(in5), _field_ptr_array(truth4),
                                              buf.stats_ptr, buf.counts_ptr, _stream_ptr(dev))
        check(rc)
        stats, counts = buf.host()
        return stats.reshape(self.models + 1, 2, 4, 4), counts

    def set_domain(self, boxes):
        """mw_surrogate_bank_set_domain: one (5, 2) box [lo, hi] per model and IN5 field (domain_box), which evaluate_domain splits the
        cells by; lo <= hi, NaN refused, +-inf allowed.  A later call replaces the boxes."""
        boxes = np.ascontiguousarray(boxes, dtype=np.float64)
        if boxes.shape != (self.models, 5, 2):
            endrun("SurrogateBank.set_domain: one (5, 2) box per model expected, (%d, 5, 2), got %r" % (self.models, boxes.shape))
        with torch.cuda.device(self.device):
            check(capi.lib().mw_surrogate_bank_set_domain(self._h, boxes.ctypes.data_as(C.POINTER(C.c_double))))
        self.boxes = boxes.copy()

    def evaluate_domain(self, nz, in5, truth4):
        """mw_surrogate_eval_domain on evaluate's arguments, after set_domain.  Returns (stats, counts): the raw (K, 2, 2, 2, 4, 4) fp64
        array [model][prediction, persistence][inside, outside][inactive, active][field][sum d, sum |d|, sum d^2, max |d|] and the int64
        cells (K, 2, 2) = [model][side][class] -- one device-to-host copy for both."""
        n, dev = self._eval_layout("SurrogateBank.evaluate_domain: ", nz, in5, truth4)
        buf = StatsAndCounts(self.models * 128, self.models * 4, dev, self._dbuf)
        self._dbuf = buf.buf
        with strict_mode(self.strict), torch.cuda.device(dev):
            rc = capi.lib().mw_surrogate_eval_domain(self._h, int(nz), n // int(nz), _field_ptr_array(in5), _field_ptr_array(truth4),
                                                     buf.stats_ptr, buf.counts_ptr, _stream_ptr(dev))
        check(rc)
        stats, counts = buf.host()
        return stats.reshape(self.models, 2, 2, 2, 4, 4), counts.reshape(self.models, 2, 2)

    def _member_layout(self, who, nz, fields):
        """(columns per member, nens) of member-fastest fields of one shape (nz, ..., nens); refuses, in the caller's name `who`, cells that
        are no whole number of columns and fields off the bank's device."""
        nens = int(fields[0].shape[-1])
        n = fields[0].numel() // nens
        if int(nz) < 1 or n % int(nz) != 0:
            endrun(who + "%d cells per member are not a whole number of columns of nz = %d" % (n, nz))
        if any(t.device != self.device for t in fields):
            endrun(who + "the bank lives on %s, the fields on %s" % (self.device, sorted({str(t.device) for t in fields})))
        return n // int(nz), nens

    def members_apply(self, nz, members, fields5):
        """mw_surrogate_members_apply: model j of the bank replaces temp and the three water fields of ensemble member members[j] of the
        coupler's member-fastest arrays fields5 = (temp, density_dry, water_vapor, cloud_liquid, precip_liquid), each (nz, ..., nens), in
        place, with the bits the forward kernels write for that member's own values (self.strict = 1: the thread-per-cell form)."""
        members = [int(m) for m in members]
        if len(members) != self.models:
            endrun("SurrogateBank.members_apply: %d members for %d models" % (len(members), self.models))
        if len(fields5) != 5 or any(t.shape != fields5[0].shape for t in fields5) or fields5[0].dim() < 2:
            endrun("SurrogateBank.members_apply: five fields of one shape (nz, ..., nens) expected")
        ncol, nens = self._member_layout("SurrogateBank.members_apply: ", nz, fields5)
        with strict_mode(self.strict), torch.cuda.device(self.device):
            rc = capi.lib().mw_surrogate_members_apply(self._h, (C.c_int * len(members))(*members), int(nz), ncol, nens,
                                                       _field_ptr_array(fields5), _stream_ptr(self.device))
        check(rc)

    def committee_apply(self, nz, sel, member, in5, out4, range4=None):
        """mw_surrogate_committee_apply: the mean of the bank's models sel (1 .. 16 distinct indices, summed in that order) on ensemble
        member `member` of the member-fastest fields in5 = (temp, density_dry, water_vapor, cloud_liquid, precip_liquid), each
        (nz, ..., nens), written to out4 = (temp, water_vapor, cloud_liquid, precip_liquid) of the same shape -- each the matching input
        tensor (in place) or a tensor of its own -- and, with range4, the members' largest minus smallest value per cell and field.  Only
        elements of `member` are read and written (self.strict = 1: the thread-per-column form)."""
        sel = [int(s) for s in sel]
        if len(in5) != 5 or len(out4) != 4 or (range4 is not None and len(range4) != 4):
            endrun("SurrogateBank.committee_apply: five input fields, four output fields and (optionally) four range fields expected")
        every = list(in5) + list(out4) + (list(range4) if range4 is not None else [])
        if any(t.shape != in5[0].shape for t in every) or in5[0].dim() < 2:
            endrun("SurrogateBank.committee_apply: fields of one shape (nz, ..., nens) expected")
        if any(t.dtype != torch.float64 or not t.is_contiguous() for t in every):
            endrun("SurrogateBank.committee_apply: contiguous float64 fields expected")
        ncol, nens = self._member_layout("SurrogateBank.committee_apply: ", nz, every)
        with strict_mode(self.strict), torch.cuda.device(self.device):
            rc = capi.lib().mw_surrogate_committee_apply(self._h, len(sel), (C.c_int * max(1, len(sel)))(*sel), int(member), int(nz), ncol, nens,
                                                         _field_ptr_array(in5), _field_ptr_array(out4),
                                                         _field_ptr_array(range4) if range4 is not None else None, _stream_ptr(self.device))
        check(rc)

    def committee_guard_flag(self, nz, sel, member, in5, thr4, guard, slot=0, domain_box=None):
        """Steps 1 and 2 of a guarded committee's step for ensemble member `member`: committee_apply of the models sel out
        of place into guard.mean4 / guard.range4, then mw_committee_guard_flags with the thresholds thr4 (temp, water_vapor, cloud_liquid,
        precip_liquid; each >= 0, inf: never by size) into guard.flags and row `slot` of guard.counts.  The state is only read.
        domain_box (a (5, 2) box, domain_box()): member_domain on that member with the guard's slot follows, so the
        columns with a cell outside the box are flagged too and the count words hold the union.  None: exactly the calls above."""
        if len(in5) != 5 or len(thr4) != 4:
            endrun("SurrogateBank.committee_guard_flag: five input fields and four thresholds expected")
        ncol, nens = self._member_layout("SurrogateBank.committee_guard_flag: ", nz, list(in5))
        guard.check_layout("SurrogateBank.committee_guard_flag: ", nz, in5[0], slot)
        self.committee_apply(nz, sel, member, in5, guard.mean4, guard.range4)
        thr = (C.c_double * 4)(*[float(t) for t in thr4])
        with torch.cuda.device(self.device):
            rc = capi.lib().mw_committee_guard_flags(int(nz), ncol, nens, int(member), _field_ptr_array(guard.mean4), _field_ptr_array(guard.range4),
                                                     thr, C.c_void_p(guard.flags.data_ptr()), C.c_void_p(guard.counts[slot].data_ptr()),
                                                     _stream_ptr(self.device))
        check(rc)
        guard.flagged_members.add(int(member))
        if domain_box is not None:
            guard.domain_counts = member_domain(nz, in5, [member], [domain_box], guard.domain_counts, guard, [slot])

    def committee_guard_apply(self, nz, sel, member, in5, thr4, max_rainsplit, dz, dt, scratch, domain_box=None):
        """One step of a guarded committee on ensemble member `member` of the member-fastest fields in5 = (temp, density_dry, water_vapor,
        cloud_liquid, precip_liquid), each (nz, ..., nens), in place: the committee's mean (committee_apply of the models sel) where its
        models agree, Kessler where they do not.  In order: committee_apply out of place into the scratch's mean4 and range4; column flags
        (some level has !(range <= thr4[f]) or a non-finite mean); mw_kessler_columns_teacher on the flagged columns of the state with
        out4 = mean4 -- the bits Kessler leaves on those columns alone, rain sub-cycles from them alone, at most max_rainsplit or the
        member's Kessler part is skipped; mw_members_copy of mean4 into the four fields.  density_dry and every other member are never
        written.  scratch: a CommitteeGuard for fields of this shape -- eight fields of the state's shape (64 bytes per element of ALL
        members, allocated once), one flag byte per column and member, the columns teacher's workspace and two int64 counts per slot.
        No host synchronisation; scratch.read(dt) fetches the counts.  A scratch used for another member before has that member's flag bytes
        cleared first: the columns teacher runs on every flagged column of the state, whichever member it belongs to.  domain_box:
        committee_guard_flag's keyword (columns outside the box go to Kessler too)."""
        if scratch.flagged_members - {int(member)}:
            scratch.flags.zero_()
            scratch.flagged_members.clear()
        self.committee_guard_flag(nz, sel, member, in5, thr4, scratch, domain_box=domain_box)
        scratch.commit(nz, [member], in5, max_rainsplit, dz, dt)


GUARD_KEYS = OUT4 + ("max_rainsplit", "domain")
DOMAIN_KEYS = ("margin", "fields")
DOMAIN_CLASSES = ("below", "above", "nan")
STENCIL_ABOVE = {0: 5, 2: 6, 3: 7, 4: 8}     # the stencil model's row of the level above, per IN5 field that has one (mlp.stencil_features)


def domain_config(d, who="domain"):
    """A checked training-domain criterion: True -- margin 0.0, all five fields of IN5 -- or a mapping with `margin` (a
    number >= 0, not a bool: the box grows by margin times its width on both sides) and `fields` (a non-empty list of distinct IN5
    names; a field left out is never outside).  Unknown keys and anything else are refused (ValueError).  Returns {"margin": float,
    "fields": [names in IN5's order]} -- pure Python."""
    if d is True:
        d = {}
    if not isinstance(d, dict):
        raise ValueError("ERROR: %s must be true or a mapping" % who)
    unknown = sorted(set(d) - set(DOMAIN_KEYS), key=str)
    if unknown:
        raise ValueError("ERROR: unknown key(s) %s in %s (known: %s)" % (", ".join(map(repr, unknown)), who, ", ".join(DOMAIN_KEYS)))
    m = d.get("margin", 0.0)
    if isinstance(m, bool) or not isinstance(m, (int, float)) or not m >= 0 or m == float("inf"):
        raise ValueError("ERROR: %s.margin must be a finite number >= 0, got %r" % (who, m))
    fields = d.get("fields", list(IN5))
    if not isinstance(fields, (list, tuple)) or not fields or any(not isinstance(f, str) or f not in IN5 for f in fields) or \
            len(set(fields)) != len(fields):
        raise ValueError("ERROR: %s.fields must be a non-empty list of distinct names of %s, got %r" % (who, ", ".join(IN5), fields))
    return {"margin": float(m), "fields": [f for f in IN5 if f in fields]}


def domain_box(models, margin=0.0, fields=IN5, names=None, tables=None):
    """The box of a model or a committee: (5, 2) fp64 [lo, hi] per IN5 field from the rows of the models' input scaling
    tables, which are the minimum and maximum of each input over the training samples.  A single-cell model gives its rows; a stencil
    model's temp, water_vapor, cloud_liquid and precip_liquid take the intersection of the cell's row and the row of the level above
    (one interval per field at every level: at level 0, whose "level above" the network never sees below it, stricter than necessary);
    several models the intersection over them.  Then [lo - margin * (hi - lo), hi + margin * (hi - lo)] in fp64 as written, and
    [-inf, +inf] for a field not in `fields`.  An empty intersection is refused (ValueError) with the field's and the models' names
    (names: theirs, default model0, model1, ...).
    tables: None, or per model None or its training-domain table (mlp.load_training_domain: the union of what the model and the models it
    continues were trained on), which then stands in for that model's scaling rows; it may be narrower than they are."""
    models = [as_surrogate_model(m) for m in models]
    if not models:
        raise ValueError("ERROR: domain_box: no models")
    names = ["model%d" % k for k in range(len(models))] if names is None else [str(n) for n in names]
    if tables is not None and len(tables) != len(models):
        raise ValueError("ERROR: domain_box: %d tables for %d models (one per model, None where it has none)" % (len(tables), len(models)))
    own = [None] * len(models) if tables is None else list(tables)
    for m, t, n in zip(models, own, names):
        if t is not None and np.shape(t) != np.shape(m.scl_in):
            raise ValueError("ERROR: domain_box: the training-domain table of model %s is %r, its input scaling table %r"
                             % (n, np.shape(t), np.shape(m.scl_in)))
    tables = [np.asarray(m.scl_in if t is None else t, dtype=np.float64) for m, t in zip(models, own)]
    if len({t.shape for t in tables}) != 1 or tables[0].ndim != 2 or tables[0].shape[1] != 2 or tables[0].shape[0] not in (5, 9):
        raise ValueError("ERROR: domain_box: the models' input scaling tables must be all (5, 2) or all (9, 2)")
    if not (isinstance(margin, (int, float)) and not isinstance(margin, bool) and 0 <= margin < float("inf")):
        raise ValueError("ERROR: domain_box: margin must be a finite number >= 0, got %r" % (margin,))
    fields = [str(f) for f in fields]
    if any(f not in IN5 for f in fields):
        raise ValueError("ERROR: domain_box: fields must be names of %s" % ", ".join(IN5))
    box = np.empty((5, 2), dtype=np.float64)
    m = np.float64(margin)
    for f, fname in enumerate(IN5):
        if fname not in fields:
            box[f] = (-np.inf, np.inf)
            continue
        rows = [t[f] for t in tables] + ([t[STENCIL_ABOVE[f]] for t in tables] if tables[0].shape[0] == 9 and f in STENCIL_ABOVE else [])
        lo, hi = np.float64(max(r[0] for r in rows)), np.float64(min(r[1] for r in rows))
        if not lo <= hi:
            raise ValueError("ERROR: domain_box: the input ranges of field %s of the models %s do not intersect (lo %r > hi %r, or NaN)"
                             % (fname, ", ".join(names), float(lo), float(hi)))
        w = hi - lo
        box[f] = (lo - m * w, hi + m * w)
    return box


def guard_config(guard, who="guard"):
    """A committee's checked guard: a mapping with any of temp, water_vapor, cloud_liquid, precip_liquid -- the range above which a column
    goes to Kessler, a number >= 0 in the field's units, a missing field never flags by size -- max_rainsplit (1 .. 1024, default 64)
    and domain (domain_config: columns with a cell outside the models' training box go to Kessler too).  Unknown keys, a
    negative, NaN or non-numeric threshold and a guard with neither a threshold nor a domain are refused (ValueError).  Returns
    {"temp", "water_vapor", "cloud_liquid", "precip_liquid": floats (inf where missing), "max_rainsplit": int} and, only when the guard
    has one, "domain": the checked criterion -- pure Python."""
    if not isinstance(guard, dict):
        raise ValueError("ERROR: %s must be a mapping" % who)
    unknown = sorted(set(guard) - set(GUARD_KEYS), key=str)
    if unknown:
        raise ValueError("ERROR: unknown key(s) %s in %s (known: %s)" % (", ".join(map(repr, unknown)), who, ", ".join(GUARD_KEYS)))
    if not any(f in guard for f in OUT4) and "domain" not in guard:
        raise ValueError("ERROR: %s holds no threshold (one of %s) and no domain" % (who, ", ".join(OUT4)))
    out = {}
    for f in OUT4:
        t = guard.get(f, float("inf"))
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not t >= 0:
            raise ValueError("ERROR: %s.%s must be a number >= 0, got %r" % (who, f, t))
        out[f] = float(t)
    cap = guard.get("max_rainsplit", 64)
    if isinstance(cap, bool) or not isinstance(cap, int) or not 1 <= cap <= 1024:
        raise ValueError("ERROR: %s.max_rainsplit must be an integer in [1, 1024], got %r" % (who, cap))
    out["max_rainsplit"] = cap
    if "domain" in guard:
        out["domain"] = domain_config(guard["domain"], who + ".domain")
    return out


def member_domain(nz, in5, members, boxes, counts=None, guard=None, slots=None):
    """mw_member_domain on the member-fastest fields in5 = (temp, density_dry, water_vapor, cloud_liquid, precip_liquid), each
    (nz, ..., nens), contiguous fp64: for member members[j] and its box boxes[j] ((5, 2) [lo, hi], domain_box) the cells of every field
    below the box, above it or NaN and the member's outside columns.  Returns the DEVICE int64 tensor (len(members), 16) -- word 3 f + c
    for field f and class c of DOMAIN_CLASSES, word 15 the outside columns -- written into `counts` if given; the call SETs it, reads
    nothing back and does not synchronise.  With guard (a CommitteeGuard) and slots (one per member, -1: none) the outside columns of
    a member with a slot get their byte of guard.flags set to 1, and both words of row slots[j] of guard.counts grow by the bytes this
    call turned from 0 to 1; the member is then added to guard.flagged_members."""
    members = [int(m) for m in members]
    boxes = np.ascontiguousarray(boxes, dtype=np.float64)
    if len(in5) != 5 or any(t.shape != in5[0].shape for t in in5) or in5[0].dim() < 2:
        endrun("member_domain: five fields of one shape (nz, ..., nens) expected")
    if any(t.dtype != torch.float64 or not t.is_contiguous() or t.device != in5[0].device for t in in5):
        endrun("member_domain: contiguous float64 fields of one device expected")
    nens, dev = int(in5[0].shape[-1]), in5[0].device
    n = in5[0].numel() // nens
    if int(nz) < 1 or n % int(nz) != 0:
        endrun("member_domain: %d cells per member are not a whole number of columns of nz = %d" % (n, nz))
    if not 1 <= len(members) <= capi.MW_DOMAIN_MAX_MEMBERS or boxes.shape != (len(members), 5, 2):
        endrun("member_domain: 1 to %d members and one (5, 2) box for each expected" % capi.MW_DOMAIN_MAX_MEMBERS)
    if counts is None:
        counts = torch.empty((len(members), capi.MW_DOMAIN_WORDS), dtype=torch.int64, device=dev)
    if tuple(counts.shape) != (len(members), capi.MW_DOMAIN_WORDS) or counts.dtype != torch.int64 or not counts.is_contiguous() or counts.device != dev:
        endrun("member_domain: counts must be a contiguous int64 tensor (%d, %d) on the fields' device" % (len(members), capi.MW_DOMAIN_WORDS))
    flags = fcounts = cslots = None
    if guard is not None or slots is not None:
        if guard is None or slots is None or len(slots) != len(members):
            endrun("member_domain: a guard and one slot per member go together")
        slots = [int(s) for s in slots]
        guard.check_layout("member_domain: ", nz, in5[0], max([0] + slots))
        flags, fcounts = C.c_void_p(guard.flags.data_ptr()), C.c_void_p(guard.counts.data_ptr())
        cslots = (C.c_int * len(slots))(*slots)
    with torch.cuda.device(dev):
        check(capi.lib().mw_member_domain(int(nz), n // int(nz), nens, len(members), (C.c_int * len(members))(*members),
                                          boxes.ctypes.data_as(C.POINTER(C.c_double)), _field_ptr_array(list(in5)), C.c_void_p(counts.data_ptr()),
                                          flags, cslots, fcounts, _stream_ptr(dev)))
    if guard is not None:
        guard.flagged_members.update(m for m, s in zip(members, slots) if s >= 0)
    return counts


class CommitteeGuard:
    """What the guarded committees of one state share (no reference counterpart): mean4 and range4, eight member-fastest scratch fields of
    the state's shape (nz, ..., nens) -- 64 bytes per element of all members, allocated here once; flags, one byte per column and member
    (zero for members that are not guarded: mw_committee_guard_flags writes its own member's bytes only); the columns teacher's workspace;
    counts, int64 (slots, 2): per guarded member this step's flagged columns and their running total."""

    def __init__(self, like, nz, slots=1):
        if like.dim() < 2 or like.dtype != torch.float64 or not like.is_contiguous() or int(nz) < 2 or like.numel() % (int(nz) * like.shape[-1]) != 0:
            endrun("CommitteeGuard: a contiguous float64 field (nz, ..., nens) with nz >= 2 expected")
        self.nz, self.nens, self.shape, self.device = int(nz), int(like.shape[-1]), tuple(like.shape), like.device
        self.ncol = like.numel() // (self.nz * self.nens)
        nbytes = capi.lib().mw_kessler_columns_teacher_workspace_bytes(self.nz, self.ncol, self.nens)
        if nbytes <= 0:
            endrun("CommitteeGuard: nz = %d, %d columns and %d members are out of range (nz >= 2, at most 64 members)" % (self.nz, self.ncol, self.nens))
        self.mean4 = [torch.empty_like(like) for _ in range(4)]
        self.range4 = [torch.empty_like(like) for _ in range(4)]
        self.flags = torch.zeros(self.ncol * self.nens, dtype=torch.uint8, device=like.device)
        self.counts = torch.zeros((int(slots), 2), dtype=torch.int64, device=like.device)
        self.workspace = fit_workspace(None, nbytes, like.device)
        self.max_rainsplit = None                                         # of the last commit (read() decides the counts with it)
        self.flagged_members = set()                                      # the members whose flag bytes may be set
        self.domain_counts = None                                         # committee_guard_flag's mw_member_domain counts, device (1, 16)

    def check_layout(self, who, nz, field, slot=0):
        if int(nz) != self.nz or tuple(field.shape) != self.shape or field.device != self.device or not 0 <= int(slot) < self.counts.shape[0]:
            endrun(who + "the CommitteeGuard was made for fields %r of nz = %d on %s with %d slot(s)" % (self.shape, self.nz, self.device, self.counts.shape[0]))

    def commit(self, nz, members, in5, max_rainsplit, dz, dt, copy=True):
        """Steps 3 to 5 for the guarded members `members`, whose mean4 and flags are in place: ONE mw_kessler_columns_teacher call on every
        flagged column of the state in5 with out4 = mean4, then mw_members_copy of the members' mean4 into temp and the three water fields
        (copy=False: the result stays in mean4 and the state is not written)."""
        self.check_layout("CommitteeGuard.commit: ", nz, in5[0])
        members = [int(m) for m in members]
        L = capi.lib()
        with torch.cuda.device(self.device):
            st = _stream_ptr(self.device)
            check(L.mw_kessler_columns_teacher(self.nz, self.ncol, self.nens, C.c_void_p(self.flags.data_ptr()), float(dz), float(dt), int(max_rainsplit),
                                               _field_ptr_array(list(in5)), _field_ptr_array(self.mean4), None, _ptr(self.workspace), st))
            if copy:
                check(L.mw_members_copy(self.nz * self.ncol, self.nens, len(members), (C.c_int * max(1, len(members)))(*members), 4,
                                        _field_ptr_array(self.mean4), _field_ptr_array([in5[0], in5[2], in5[3], in5[4]]), st))
        self.max_rainsplit = int(max_rainsplit)

    def read(self, dt, members=(0,)):
        """After a commit, with two small device-to-host copies: per slot (flagged columns of the last step, their running total), and the
        rain sub-cycle count of each of `members` in that step (0: its Kessler part was skipped)."""
        counts = self.counts.cpu().numpy()
        words = self.workspace[:self.nens].cpu().numpy().view(np.uint64)
        dt_bits = int(np.float64(dt).view(np.uint64))
        rs = []
        for m in members:
            w = min(int(words[int(m)]), dt_bits)                          # a word no column lowered stands for dt (kessler_teacher_word)
            rs.append(int(capi.lib().mw_kessler_teacher_rainsplit(float(dt), float(np.uint64(w).view(np.float64)), int(self.max_rainsplit))))
        return [(int(a), int(b)) for a, b in counts], rs


def json_safe(x):
    """Nested lists of floats with inf / NaN as the strings "inf", "-inf", "nan" (bare tokens are no JSON); finite numbers unchanged."""
    if isinstance(x, list):
        return [json_safe(v) for v in x]
    return x if np.isfinite(x) else str(float(x))


def box_json(box):
    """A (5, 2) box as {field: [lo, hi]} with inf as a string (json_safe)."""
    return {f: json_safe([float(box[i][0]), float(box[i][1])]) for i, f in enumerate(IN5)}


def finite_or_none(row, bad=False):
    """A report's row of statistics (numbers or None): unchanged when every number is finite and `bad` is not set; else the row with None
    for each statistic that is inf or NaN (a diverged model) and "finite": False behind them."""
    if not bad and all(x is None or np.isfinite(x) for x in row.values()):
        return row
    row = {k: (x if x is not None and np.isfinite(x) else None) for k, x in row.items()}
    row["finite"] = False
    return row


def or_dash(x, fmt):
    return "-" if x is None else fmt % x


def skill_cell(rmse, ratio):
    """The cell of a skill table: the rmse and, in brackets, the rmse over the persistence row's."""
    return "%26s" % ("-" if rmse is None else "%.6e (%s)" % (rmse, or_dash(ratio, "%.4g")))


def _exact_sum_units(x):
    n, d = float(x).as_integer_ratio()
    return n * (_EXACT_ONE // d)


def _exact_units_array(x):
    """An fp64 array as (exact integers in units of 2^-1074, the non-finite values apart): a sum that is inf or NaN lives in the second
    array and its integer is 0."""
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x)
    units = np.zeros(x.shape, dtype=object)
    flat, ff, src = units.reshape(-1), fin.reshape(-1), x.reshape(-1)
    for i in range(flat.size):
        flat[i] = _exact_sum_units(src[i]) if ff[i] else 0
    return units, np.where(fin, 0.0, x)


def surrogate_scores(stats, counts):
    """One raw result of SurrogateBank.evaluate as the accumulating form SurrogateEvaluator.combine adds: `sums` (K + 1, 2, 4, 3) exact
    integers in units of 2^-1074, `nonfinite` the same shape in fp64 (a sum that is inf or NaN -- a diverged model -- lives here and its
    integer is 0), `max` (K + 1, 2, 4), `counts` (2,) and the number of calls."""
    stats = np.asarray(stats, dtype=np.float64)
    sums, nonfinite = _exact_units_array(stats[..., :3])
    return {"sums": sums, "nonfinite": nonfinite, "max": stats[..., 3].copy(), "counts": np.asarray(counts, dtype=np.int64).copy(), "calls": 1}


def _sums_to_float(sums, nonfinite):
    out = np.array([v / _EXACT_ONE for v in sums.reshape(-1)], dtype=np.float64).reshape(sums.shape)      # int / int: correctly rounded
    return np.where(nonfinite != 0.0, nonfinite, out)


class SurrogateEvaluator:
    """Scores every model of several banks (one per width) against the microphysics in charge, call after call: accumulate(inp, out) with
    the coupler cloned before micro.time_step and the stepped one (the pair gather_micro_statistics takes), report() at the end.
    names: the models' names, bank after bank."""

    def __init__(self, banks, names):
        self.banks = list(banks)
        self.names = [str(n) for n in names]
        if len(self.names) != sum(b.models for b in self.banks):
            endrun("SurrogateEvaluator: %d names for %d models" % (len(self.names), sum(b.models for b in self.banks)))
        if len(set(self.names)) != len(self.names):
            endrun("SurrogateEvaluator: model names must be unique")
        self.total = None
        self.history = []               # per call: the raw statistics and counts of every bank

    @staticmethod
    def combine(a, b):
        """Two results (lists with one surrogate_scores dict per bank) as one: sums add, maxima take the larger, counts and calls add.  The
        sums are exact integers, so the order of combination cannot matter: (a + b) + c == a + (b + c), also across ranks; by convention
        `a` is the earlier result."""
        if len(a) != len(b):
            endrun("SurrogateEvaluator.combine: results of different evaluators")
        out = []
        for x, y in zip(a, b):
            if x["sums"].shape != y["sums"].shape:
                endrun("SurrogateEvaluator.combine: results of different banks")
            out.append({"sums": x["sums"] + y["sums"], "nonfinite": x["nonfinite"] + y["nonfinite"], "max": np.maximum(x["max"], y["max"]),
                        "counts": x["counts"] + y["counts"], "calls": x["calls"] + y["calls"]})
        return out

    def accumulate(self, inp, out):
        """Runs every bank on (inp, out) and adds the call to the running total; returns the call's own result."""
        in5 = [inp.get_data_manager_readonly().get(n, True) for n in IN5]
        truth4 = [out.get_data_manager_readonly().get(n, True) for n in EVAL_FIELDS]
        raw = [bank.evaluate(inp.get_nz(), in5, truth4) for bank in self.banks]
        self.history.append([{"stats": json_safe(s.tolist()), "counts": c.tolist()} for s, c in raw])
        one = [surrogate_scores(s, c) for s, c in raw]
        self.total = one if self.total is None else self.combine(self.total, one)
        return one

    def report(self, result=None):
        """Per model (and `persistence:<bank>`), per class (inactive, active, all) and field: n, bias = sum d / n, mae, rmse, max_abs and
        rmse_over_persistence (the skill's denominator: the same class and field of the bank's persistence row).  An empty class has n = 0
        and None for every statistic; so has a ratio whose persistence rmse is 0.  A statistic that is inf or NaN (a diverged model: NaN reaches
        the sums AND max_abs) is None too, and its field carries "finite": False."""
        result = self.total if result is None else result
        if result is None:
            endrun("SurrogateEvaluator.report: nothing accumulated")
        rep, first = {}, 0
        for ib, (bank, r) in enumerate(zip(self.banks, result)):
            sums, nonf = r["sums"], r["nonfinite"]
            # class axis -> (inactive, active, all)
            s3 = _sums_to_float(np.concatenate([sums, sums.sum(axis=1, keepdims=True)], axis=1),
                                np.concatenate([nonf, nonf.sum(axis=1, keepdims=True)], axis=1))
            mx = np.concatenate([r["max"], r["max"].max(axis=1, keepdims=True)], axis=1)
            n = np.concatenate([r["counts"], [r["counts"].sum()]]).astype(np.float64)
            some = n > 0
            with np.errstate(divide="ignore", invalid="ignore"):
                per = s3 / np.where(some, n, 1.0)[None, :, None, None]
                rmse = np.sqrt(per[..., 2])
                skill = rmse / rmse[-1:]
            ok_skill = some[None, :, None] & (rmse[-1:] > 0)
            for m in range(bank.models + 1):
                name = self.names[first + m] if m < bank.models else "persistence:%d" % ib
                rep[name] = {}
                for c, cname in enumerate(EVAL_CLASSES + ("all",)):
                    row = {"n": int(n[c])}
                    for v, fname in enumerate(EVAL_FIELDS):
                        if some[c]:
                            row[fname] = finite_or_none({"bias": float(per[m, c, v, 0]), "mae": float(per[m, c, v, 1]), "rmse": float(rmse[m, c, v]),
                                                         "max_abs": float(mx[m, c, v]),
                                                         "rmse_over_persistence": float(skill[m, c, v]) if ok_skill[0, c, v] else None})
                        else:
                            row[fname] = {"bias": None, "mae": None, "rmse": None, "max_abs": None, "rmse_over_persistence": None}
                    rep[name][cname] = row
            first += bank.models
        return rep

    def table(self, rep=None):
        """report() as text: one line per model and class, rmse / persistence rmse per field (the skill: < 1 beats doing nothing)."""
        rep = self.report() if rep is None else rep
        w = max(len(k) for k in rep)
        lines = ["%-*s %-8s %12s " % (w, "model", "class", "n") + " ".join("%26s" % ("%s rmse (/pers.)" % f) for f in EVAL_FIELDS)]
        for name, classes in rep.items():
            for cname, row in classes.items():
                cells = [skill_cell(row[f]["rmse"], row[f]["rmse_over_persistence"]) for f in EVAL_FIELDS]
                lines.append("%-*s %-8s %12d " % (w, name, cname, row["n"]) + " ".join(cells))
        return "\n".join(lines)


EVAL_SIDES = ("inside", "outside")
EVAL_DOMAIN_KEYS = DOMAIN_KEYS + ("box_of",)


def eval_domain_config(d, model_names, who="eval_domain"):
    """The checked `eval_domain:` key of evaluate_surrogates: True, or a mapping with domain_config's `margin` and
    `fields` and, optionally, `box_of`: the name of one of model_names, whose box then serves every model (a continued model and its
    parent on one partition).  Unknown keys, a box_of that names no model and what domain_config refuses are ValueErrors.  Returns
    {"margin": float, "fields": [names], "box_of": name or None} -- pure Python."""
    if d is True:
        d = {}
    if not isinstance(d, dict):
        raise ValueError("ERROR: %s must be true or a mapping" % who)
    unknown = sorted(set(d) - set(EVAL_DOMAIN_KEYS), key=str)
    if unknown:
        raise ValueError("ERROR: unknown key(s) %s in %s (known: %s)" % (", ".join(map(repr, unknown)), who, ", ".join(EVAL_DOMAIN_KEYS)))
    box_of = d.get("box_of")
    if box_of is not None and (not isinstance(box_of, str) or box_of not in [str(n) for n in model_names]):
        raise ValueError("ERROR: %s.box_of must name one of surrogate_models (%s), got %r" % (who, ", ".join(map(str, model_names)), box_of))
    return dict(domain_config({k: v for k, v in d.items() if k != "box_of"}, who), box_of=box_of)


def domain_scores(stats, counts):
    """One raw result of SurrogateBank.evaluate_domain in surrogate_scores' accumulating form: `sums` (K, 2, 2, 2, 4, 3) exact integers in
    units of 2^-1074, `nonfinite` the same shape, `max` (K, 2, 2, 2, 4), `counts` (K, 2, 2) and the number of calls."""
    return surrogate_scores(stats, counts)


def domain_split_report(names, boxes, result):
    """DomainSplitEvaluator.report from accumulated results alone -- pure numpy.  names: the models', bank after bank; boxes: their (5, 2)
    boxes; result: one domain_scores dict per bank."""
    rep, first = {}, 0
    classes = EVAL_CLASSES + ("all",)
    for r in result:
        sums, nonf, mx, cnt = r["sums"], r["nonfinite"], r["max"], r["counts"]
        # class axis (3) -> (inactive, active, all)
        sums3 = np.concatenate([sums, sums.sum(axis=3, keepdims=True)], axis=3)
        nonf3 = np.concatenate([nonf, nonf.sum(axis=3, keepdims=True)], axis=3)
        s3 = _sums_to_float(sums3, nonf3)
        mx3 = np.concatenate([mx, mx.max(axis=3, keepdims=True)], axis=3)
        n3 = np.concatenate([cnt, cnt.sum(axis=2, keepdims=True)], axis=2)                         # (K, side, 3)
        for m in range(sums.shape[0]):
            box = np.asarray(boxes[first + m], dtype=np.float64)
            entry = {"box": box_json(box)}
            for sd, sname in enumerate(EVAL_SIDES):
                entry[sname] = {}
                for c, cname in enumerate(classes):
                    n = int(n3[m, sd, c])
                    row = {"n": n}
                    for v, fname in enumerate(EVAL_FIELDS):
                        if n > 0:
                            with np.errstate(divide="ignore", invalid="ignore"):
                                per, pers = s3[m, 0, sd, c, v] / n, s3[m, 1, sd, c, v] / n
                                rmse, prmse = np.sqrt(per[2]), np.sqrt(pers[2])
                            row[fname] = finite_or_none({"bias": float(per[0]), "mae": float(per[1]), "rmse": float(rmse),
                                                         "max_abs": float(mx3[m, 0, sd, c, v]),
                                                         "rmse_over_persistence": float(rmse / prmse) if prmse > 0 else None})
                        else:
                            row[fname] = {"bias": None, "mae": None, "rmse": None, "max_abs": None, "rmse_over_persistence": None}
                    entry[sname][cname] = row
            share = {}
            for c, cname in enumerate(classes):
                share[cname] = {}
                for v, fname in enumerate(EVAL_FIELDS):
                    ins, out = int(sums3[m, 0, 0, c, v, 2]), int(sums3[m, 0, 1, c, v, 2])
                    bad = nonf3[m, 0, 0, c, v, 2] != 0.0 or nonf3[m, 0, 1, c, v, 2] != 0.0
                    share[cname][fname] = None if bad or ins + out == 0 else out / (ins + out)           # int / int: correctly rounded
            entry["outside_share_of_squared_error"] = share
            rep[str(names[first + m])] = entry
        first += sums.shape[0]
    return rep


class DomainSplitEvaluator:
    """SurrogateEvaluator with every model's errors split by inside / outside its training box: how much of a model's
    one-step error comes from extrapolation.  banks, names: SurrogateEvaluator's; boxes: one (5, 2) box per model, bank after bank
    (domain_box), handed to the banks here.  accumulate(inp, out) call after call, report() at the end; the sums are exact integers in
    units of 2^-1074, so combine is order-free."""

    def __init__(self, banks, names, boxes):
        self.banks = list(banks)
        self.names = [str(n) for n in names]
        if len(self.names) != sum(b.models for b in self.banks):
            endrun("DomainSplitEvaluator: %d names for %d models" % (len(self.names), sum(b.models for b in self.banks)))
        if len(set(self.names)) != len(self.names):
            endrun("DomainSplitEvaluator: model names must be unique")
        self.boxes = np.ascontiguousarray(boxes, dtype=np.float64)
        if self.boxes.shape != (len(self.names), 5, 2):
            endrun("DomainSplitEvaluator: one (5, 2) box per model expected, got %r" % (self.boxes.shape,))
        first = 0
        for b in self.banks:
            b.set_domain(self.boxes[first:first + b.models])
            first += b.models
        self.total = None
        self.history = []               # per call: the raw statistics and counts of every bank

    @staticmethod
    def combine(a, b):
        """SurrogateEvaluator.combine on domain_scores dicts: sums add, maxima take the larger, counts and calls add."""
        return SurrogateEvaluator.combine(a, b)

    def accumulate(self, inp, out):
        """Runs every bank's evaluate_domain on (inp, out) and adds the call to the running total; returns the call's own result."""
        in5 = [inp.get_data_manager_readonly().get(n, True) for n in IN5]
        truth4 = [out.get_data_manager_readonly().get(n, True) for n in EVAL_FIELDS]
        raw = [bank.evaluate_domain(inp.get_nz(), in5, truth4) for bank in self.banks]
        self.history.append([{"stats": json_safe(s.tolist()), "counts": c.tolist()} for s, c in raw])
        one = [domain_scores(s, c) for s, c in raw]
        self.total = one if self.total is None else self.combine(self.total, one)
        return one

    def report(self, result=None):
        """Per model: its box; per side (inside, outside), class (inactive, active, all) and field n, bias, mae, rmse, max_abs and
        rmse_over_persistence against the persistence rows of the same model, side and class; and per class and field
        outside_share_of_squared_error = sum d^2 outside / (inside + outside) from the exact integers (None when both are 0 or one is
        not finite).  Empty classes and non-finite statistics as in SurrogateEvaluator.report: None, "finite": False."""
        result = self.total if result is None else result
        if result is None:
            endrun("DomainSplitEvaluator.report: nothing accumulated")
        return domain_split_report(self.names, self.boxes, result)

    def table(self, rep=None):
        """report() as text: one line per model, side and class; rmse / persistence rmse per field, then the outside share of sum d^2."""
        rep = self.report() if rep is None else rep
        w = max(len(k) for k in rep)
        lines = ["%-*s %-8s %-8s %12s " % (w, "model", "side", "class", "n") + " ".join("%26s" % ("%s rmse (/pers.)" % f) for f in EVAL_FIELDS)]
        for name, entry in rep.items():
            for sname in EVAL_SIDES:
                for cname, row in entry[sname].items():
                    cells = [skill_cell(row[f]["rmse"], row[f]["rmse_over_persistence"]) for f in EVAL_FIELDS]
                    lines.append("%-*s %-8s %-8s %12d " % (w, name, sname, cname, row["n"]) + " ".join(cells))
            for cname, row in entry["outside_share_of_squared_error"].items():
                lines.append("%-*s %-8s %-8s %12s " % (w, name, "share", cname, "") + " ".join("%26s" % or_dash(row[f], "%.4f") for f in EVAL_FIELDS))
        return "\n".join(lines)


class _CommitteeRow:
    models = 1            # what SurrogateEvaluator.report reads of a bank: the committee is the one "model" beside the persistence row


def committee_score(nz, in5, truth4, pred4, range4, workspace=None):
    """mw_committee_score on contiguous fp64 CUDA fields of nz levels: returns (stats (2, 4, 7) fp64 = [class][field][sum d, sum |d|,
    sum d^2, max |d|, sum r, sum r^2, sum r |d|], counts (2,) int64 cells per class, covered (2, 4) int64 cells with |d| <= r), d = pred -
    truth, r = range; classes as SurrogateBank.evaluate -- one device-to-host copy."""
    every = list(in5) + list(truth4) + list(pred4) + list(range4)
    if (len(in5), len(truth4), len(pred4), len(range4)) != (5, 4, 4, 4):
        endrun("committee_score: five input fields and four truth, prediction and range fields expected")
    n, dev = in5[0].numel(), in5[0].device
    if int(nz) < 1 or n % int(nz) != 0 or any(t.numel() != n for t in every):
        endrun("committee_score: the seventeen fields must have one size, a whole number of columns of nz = %d levels" % nz)
    if any(t.device != dev or t.dtype != torch.float64 or not t.is_contiguous() for t in every):
        endrun("committee_score: contiguous float64 fields of one device expected")
    L = capi.lib()
    ws = fit_workspace(workspace, L.mw_committee_score_workspace_bytes(int(nz), n // int(nz)), dev)
    buf = StatsAndCounts(56, 10, dev)                                           # the ten counts: cells per class, then covered
    with torch.cuda.device(dev):
        check(L.mw_committee_score(int(nz), n // int(nz), _field_ptr_array(in5), _field_ptr_array(truth4), _field_ptr_array(pred4),
                                   _field_ptr_array(range4), _ptr(ws), buf.stats_ptr, buf.counts_ptr, _stream_ptr(dev)))
    stats, counts = buf.host()
    return stats.reshape(2, 4, 7), counts[:2], counts[2:].reshape(2, 4)


def range_error_correlation(n, sum_r, sum_r2, sum_a, sum_a2, sum_ra):
    """Pearson's r of the range r and the error |d| over n cells from their six sums; None when a sum is not finite or a variance is not
    positive (a constant range, a perfect prediction, an empty class)."""
    vals = (sum_r, sum_r2, sum_a, sum_a2, sum_ra)
    if n < 1 or not all(np.isfinite(v) for v in vals):
        return None
    mr, ma = sum_r / n, sum_a / n
    vr, va = sum_r2 / n - mr * mr, sum_a2 / n - ma * ma
    if not (vr > 0.0 and va > 0.0):
        return None
    q = (sum_ra / n - mr * ma) / np.sqrt(vr * va)
    return float(min(1.0, max(-1.0, q))) if np.isfinite(q) else None


class CommitteeEvaluator:
    """Scores the committee `sel` of a bank against the microphysics in charge, call after call, as SurrogateEvaluator scores single
    models: accumulate(inp, out) runs the committee forward into scratch fields (mean and range) and mw_committee_score on them, report()
    gives per class (inactive, active, all) and field the evaluator's row (bias, mae, rmse, max_abs, rmse_over_persistence) plus mean_range,
    coverage (the fraction of cells with |d| <= range) and range_error_correlation (range_error_correlation above)."""

    def __init__(self, bank, sel):
        self.bank, self.sel = bank, [int(i) for i in sel]
        if not 1 <= len(self.sel) <= capi.MW_COMMITTEE_MAX_MODELS:
            endrun("CommitteeEvaluator: a committee has 1 to %d models, got %d" % (capi.MW_COMMITTEE_MAX_MODELS, len(self.sel)))
        if len(set(self.sel)) != len(self.sel) or any(not 0 <= i < bank.models for i in self.sel):
            endrun("CommitteeEvaluator: the committee must name distinct models of the bank's %d" % bank.models)
        self.total = None
        self.history = []
        self._scratch = None
        self._ws = None

    def accumulate(self, inp, out):
        """One call: the committee's mean and range from `inp`, scored against `out`; added to the running total.  Returns the call's raw
        (stats (2, 2, 4, 7) = [committee | persistence], counts (2,), covered (2, 4))."""
        nz = inp.get_nz()
        in5 = [inp.get_data_manager_readonly().get(n, True) for n in IN5]
        truth4 = [out.get_data_manager_readonly().get(n, True) for n in EVAL_FIELDS]
        if self._scratch is None or self._scratch[0].shape != in5[0].shape:
            self._scratch = [torch.empty_like(in5[0]) for _ in range(8)]
        pred4, range4 = self._scratch[:4], self._scratch[4:]
        as1 = lambda ts: [t.reshape(nz, -1, 1) for t in ts]                     # noqa: E731   (every member is one more column)
        self.bank.committee_apply(nz, self.sel, 0, as1(in5), as1(pred4), as1(range4))
        ws = grown_workspace(self, "_ws", capi.lib().mw_committee_score_workspace_bytes(nz, in5[0].numel() // nz), in5[0].device)
        stats, counts, covered = committee_score(nz, in5, truth4, pred4, range4, ws)
        pstats, _, _ = committee_score(nz, in5, truth4, [in5[0], in5[2], in5[3], in5[4]], range4, ws)      # persistence: prediction = input
        both = np.stack([stats, pstats])
        self.history.append({"stats": json_safe(both.tolist()), "counts": counts.tolist(), "covered": covered.tolist()})
        units, nonf = _exact_units_array(stats[..., 4:])
        one = {"scores": [surrogate_scores(both[..., :4], counts)], "rsums": units, "rnonfinite": nonf, "covered": covered.astype(np.int64)}
        if self.total is None:
            self.total = one
        else:
            t = self.total
            self.total = {"scores": SurrogateEvaluator.combine(t["scores"], one["scores"]), "rsums": t["rsums"] + units,
                          "rnonfinite": t["rnonfinite"] + nonf, "covered": t["covered"] + one["covered"]}
        return both, counts, covered

    def report(self):
        if self.total is None:
            endrun("CommitteeEvaluator.report: nothing accumulated")
        t = self.total
        base = SurrogateEvaluator([_CommitteeRow()], ["committee"]).report(t["scores"])["committee"]
        sc = t["scores"][0]
        counts = np.concatenate([sc["counts"], [sc["counts"].sum()]])
        with3 = lambda a: np.concatenate([a, a.sum(axis=0, keepdims=True)], axis=0)      # noqa: E731   class axis -> (inactive, active, all)
        rs = _sums_to_float(with3(t["rsums"]), with3(t["rnonfinite"]))                 # (3, 4, 3): sum r, sum r^2, sum r |d|
        ds = _sums_to_float(with3(sc["sums"][0]), with3(sc["nonfinite"][0]))           # (3, 4, 3): sum d, sum |d|, sum d^2
        cov = with3(t["covered"])
        rep = {}
        for c, cname in enumerate(EVAL_CLASSES + ("all",)):
            n = int(counts[c])
            row = {"n": n}
            for v, fname in enumerate(EVAL_FIELDS):
                f = dict(base[cname][fname])
                if n > 0:
                    mr = rs[c, v, 0] / n
                    f["mean_range"] = float(mr) if np.isfinite(mr) else None
                    f["coverage"] = int(cov[c, v]) / n
                    f["range_error_correlation"] = range_error_correlation(n, rs[c, v, 0], rs[c, v, 1], ds[c, v, 1], ds[c, v, 2], rs[c, v, 2])
                    if f["mean_range"] is None:
                        f["finite"] = False
                else:
                    f.update(mean_range=None, coverage=None, range_error_correlation=None)
                row[fname] = f
            rep[cname] = row
        return rep

    def table(self, rep=None, name="committee"):
        """report() as text: one line per class; rmse / persistence rmse, mean range and coverage per field."""
        rep = self.report() if rep is None else rep
        lines = ["%-16s %-8s %12s " % ("committee", "class", "n") + " ".join("%40s" % ("%s rmse (/pers.) range cover" % f) for f in EVAL_FIELDS)]
        for cname, row in rep.items():
            cells = ["%40s" % ("%s (%s) %s %s" % (or_dash(row[f]["rmse"], "%.4e"), or_dash(row[f]["rmse_over_persistence"], "%.4g"),
                                                   or_dash(row[f]["mean_range"], "%.3e"), or_dash(row[f]["coverage"], "%.3f"))) for f in EVAL_FIELDS]
            lines.append("%-16s %-8s %12d " % (name, cname, row["n"]) + " ".join(cells))
        return "\n".join(lines)
