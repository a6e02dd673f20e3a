"""Range guard of the f16mx operands (MODEL.HIP.MX_RANGE_GUARD).

An f16mx activation carries no scale (csrc/f16mx.h): its fp16 `hi` plane is +-inf beyond 65504, its e4m3 planes are clamped at
+-448, and a trained weight keeps the scale byte of its last full encode.  The fp32 reference has no such cliff.  The guard
counts, per named SITE (a producer of f16mx bytes), what the audit kernel (wsovod_f16mx_range) finds in the bytes the producers
already wrote:

    audited    values looked at
    nonfinite  values whose hi is inf / NaN: the product itself is lost
    top_code   values whose q byte is the format's top code: |x 2^-s| >= 432 rounded to 448 or was clamped there -- the e4m3
               cross terms of these values are wrong, products fall back to fp16 grade (2^-11); conservative: 432 .. 448 is
               still represented to e4m3's own half ulp
    max_abs    the largest finite |hi|

All rows live in ONE device tensor; `poll` reads it with one device-to-host copy.  Audits are launched only while the guard is
ARMED and is the ACTIVE guard of the calling thread (`active`; the armed flag and the table belong to the one guard object of
a model and are not synchronised between threads): the model code calls the module-level `audit` where a carrier
is produced, which costs one attribute read when no guard is active.  Importable without the HIP library.
"""
import contextlib
import logging
import threading
from collections import namedtuple

import numpy as np
import torch

from .precision import TABLE

MODES = ("off", "warn", "raise", "fallback")
MX_PRECISIONS = tuple(n for n, p in TABLE.items() if p.mx)  # the names with f16mx operands
MAX_SITES = 256

SiteReport = namedtuple("SiteReport", "audited nonfinite top_code max_abs")

_log = logging.getLogger(__name__)


def _tripped(r):
    return r.nonfinite != 0 or r.top_code != 0


def build_report(names, table):
    """{site: SiteReport} of a host (len(names), 4) int64 table; [3] is an fp16 bit pattern."""
    rows = np.asarray(table, dtype=np.int64).reshape(-1, 4)
    return {n: SiteReport(int(r[0]), int(r[1]), int(r[2]), float(np.array([int(r[3]) & 0x7FFF], dtype=np.uint16).view(np.float16)[0]))
            for n, r in zip(names, rows)}


def tripping(report):
    """The sites of `report` with a non-finite or top-code count, in audit order."""
    return [n for n, r in report.items() if _tripped(r)]


class MxRangeError(RuntimeError):
    """An f16mx operand left the format's range.  `report`: {site: SiteReport}; `site`: the first one that tripped."""

    def __init__(self, report, what="f16mx operand out of range"):
        self.report = report
        bad = tripping(report)
        self.site = bad[0] if bad else None
        r = report.get(self.site)
        detail = "" if r is None else (f" at site '{self.site}': {r.nonfinite} non-finite hi, {r.top_code} values at the q plane's "
                                       f"top code (|x| >= 432 x scale) of {r.audited}, largest finite |hi| {r.max_abs:g}"
                                       + (f"; {len(bad) - 1} more site(s)" if len(bad) > 1 else ""))
        super().__init__(f"wsovod_hip MX_RANGE_GUARD: {what}{detail}")


class MxRangeGuard:
    def __init__(self, mode="raise", period=100, names=None):
        if mode not in MODES or mode == "off":
            raise ValueError(f"MxRangeGuard: mode must be one of {MODES[1:]}, got {mode!r}")
        if int(period) < 1:
            raise ValueError(f"MODEL.HIP.MX_RANGE_GUARD_PERIOD must be >= 1, got {period}")
        self.mode, self.period = mode, int(period)
        self.names = dict(names or {})  # id(module) -> site name (a module may be given as the site)
        self.sites = {}                 # site name -> row of the table, in first-audit order
        self.table = None               # (MAX_SITES, 4) int64 on the device of the first audited tensor
        self.totals = {}                # site -> values audited over all polls (host side)
        self.polls = 0
        self.last = {}                  # the report of the last poll
        self.fallen_back = False        # "fallback" tripped: the model runs the bf16x2 kernels from now on
        self._armed = False
        self._since = 0                 # training steps since the last forced arm (construction, a state-dict load)
        self._warned = set()

    # ---- arming ----
    def arm(self, on=True):
        self._armed = bool(on) and not self.fallen_back
        return self._armed

    def armed(self):
        return self._armed

    def rearm(self):
        """A state dict was loaded: the next training step is audited whatever the period says."""
        self._since = 0

    def begin_step(self):
        """Training: arm the first step and every `period`-th after it (with a cleared table) -> armed."""
        due = self._since % self.period == 0
        self._since += 1
        if self.arm(due):
            self.reset()
        return self._armed

    # ---- the table ----
    def _row(self, site, device):
        if self.table is None:
            self.table = torch.zeros((MAX_SITES, 4), dtype=torch.int64, device=device)
        name = site if isinstance(site, str) else self.names.get(id(site))
        if name is None:
            name = f"{type(site).__name__}@{len(self.sites)}"
            self.names[id(site)] = name
        row = self.sites.get(name)
        if row is None:
            if len(self.sites) >= MAX_SITES:
                raise RuntimeError(f"MxRangeGuard: more than {MAX_SITES} sites")
            row = self.sites[name] = len(self.sites)
        return self.table[row]

    def audit(self, site, tensor, operand=False):
        """Armed: count `tensor`'s range into `site`'s row (one kernel launch, no host read).  operand: a weight's f16mx
        operand carrier (scaled; never tagged) instead of a tagged activation."""
        if not self._armed:
            return
        from . import hip_ops as H

        H.mx_range(tensor, self._row(site, tensor.device), operand=operand)

    def reset(self):
        if self.table is not None:
            self.table.zero_()

    def poll(self):
        """ONE device-to-host read -> {site: SiteReport} of the counts since the last reset."""
        self.polls += 1
        if self.table is None or not self.sites:
            self.last = {}
            return self.last
        rep = self.last = build_report(list(self.sites), self.table[:len(self.sites)].cpu().numpy())
        for n, r in rep.items():
            self.totals[n] = self.totals.get(n, 0) + r.audited
        return rep

    # ---- the decision ----
    def settle(self, report, updated=False, training=False):
        """Act on a polled report by the mode -> "ok", "warn" or "fallback"; raises MxRangeError under "raise".  training: the
        report is a training step's ("fallback" then means from the NEXT step; an inference call re-runs its batch); updated:
        that step has applied its optimizer update already -- a non-finite hi then raises in every mode."""
        self._armed = False
        bad = tripping(report)
        if not bad:
            return "ok"
        if updated and any(report[n].nonfinite for n in bad):
            raise MxRangeError(report, "a non-finite f16mx value went into an optimizer step that is already applied")
        if self.mode == "raise":
            raise MxRangeError(report)
        err = MxRangeError(report)
        if self.mode == "fallback":
            self.fallen_back = True
            _log.warning("%s -- %s", err, "this step used saturated cross terms; the bf16x2 kernels (\"parity\") run from the next "
                         "step" if (training or updated) else
                         "re-running this batch on the bf16x2 kernels (\"parity\"), which later calls use too")
            return "fallback"
        for n in bad:
            if n not in self._warned:
                self._warned.add(n)
                r = report[n]
                _log.warning("wsovod_hip MX_RANGE_GUARD: site '%s': %d non-finite hi, %d of %d values at the q plane's top code "
                             "(products of these fall to fp16 grade), largest finite |hi| %g", n, r.nonfinite, r.top_code,
                             r.audited, r.max_abs)
        return "warn"


def from_config(cfg):
    """The guard MODEL.HIP.MX_RANGE_GUARD asks for, None for "off"; refuses a precision without f16mx operands."""
    hip = cfg.MODEL.HIP
    mode, period = hip.MX_RANGE_GUARD, hip.MX_RANGE_GUARD_PERIOD
    if mode not in MODES:
        raise ValueError(f"MODEL.HIP.MX_RANGE_GUARD must be one of {MODES}, got {mode!r}")
    if mode == "off":
        return None
    if hip.PRECISION not in MX_PRECISIONS:
        raise ValueError(f'MODEL.HIP.MX_RANGE_GUARD = "{mode}" guards f16mx operands: it needs MODEL.HIP.PRECISION in '
                         f'{MX_PRECISIONS}, got "{hip.PRECISION}"')
    return MxRangeGuard(mode, period)


# ---- the active guard of a thread: audit calls reach a guard only from inside a model entry point of that thread.  The guard
# OBJECT (armed flag, table, reset) is one per model and not synchronised: inference() on a model from a second thread WHILE
# the first runs a training step on it arms and clears the same table -- the trainer's own eval / TTA hooks run between steps,
# on the training thread, which is the supported use ----
class _Active(threading.local):
    guard = None


_ACTIVE = _Active()


@contextlib.contextmanager
def active(guard):
    prev, _ACTIVE.guard = _ACTIVE.guard, guard
    try:
        yield guard
    finally:
        _ACTIVE.guard = prev


def launching():
    """True while audits are being launched on this thread (such a forward is neither captured nor replayed)."""
    g = _ACTIVE.guard
    return g is not None and g._armed


def audit(site, tensor, operand=False):
    g = _ACTIVE.guard
    if g is not None and g._armed:
        g.audit(site, tensor, operand=operand)
