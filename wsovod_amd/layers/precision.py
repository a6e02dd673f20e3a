"""MODEL.HIP.PRECISION in one place: what every name means (`TABLE`, `of`) and the calling thread's live state -- the x3 mode,
the f16mx selection, the backward split -- with the scopes that set it.  Pure Python: importable without the HIP library."""
import os
import threading
from dataclasses import dataclass

import torch


@dataclass(frozen=True)
class Precision:
    name: str                # the config name
    forward: str             # the name the modules see: a composite name is the "parity" forward plus the flags below
    x3: object = False       # the x3_mode of the model's entry points: False, "full", "fwd" or "x2"
    mx: bool = False         # the big forward contractions take the f16mx kernels (mx_mode)
    bwd_split: bool = False  # the backward keeps the hi/lo split (backward_split)

    @property
    def x3_float_entry(self):
        return "fwd" if self.x3 == "x2" else self.x3  # the backbones' float entry has no bf16x2 first conv: "x2" runs as "fwd"

    @property
    def compute_dtype(self):
        return torch.bfloat16 if self.forward == "bf16" else torch.float32  # "fp32", the x3 modes and "parity": fp32 tensors


TABLE = {p.name: p for p in (
    Precision("bf16", "bf16"),
    Precision("fp32", "fp32"),
    Precision("bf16x3", "bf16x3", "full"),
    Precision("bf16x3f", "bf16x3f", "fwd"),
    Precision("parity", "parity", "x2"),
    Precision("parity_train", "parity", "x2", bwd_split=True),
    Precision("parity_mx", "parity", "x2", mx=True),
    Precision("parity_mx_train", "parity", "x2", mx=True, bwd_split=True),
)}


def of(name):
    """The table's record of `name`; a name the project does not know is handed through: fp32 tensors, no flags."""
    return TABLE.get(name) or Precision(name, name)


class _State(threading.local):
    """Per-thread: a TTA / data-loader thread must neither see nor clobber the mode of the autograd thread."""
    x3 = False
    mx = False
    bwd_split = False


_STATE = _State()


class _Scope:
    """Context manager: sets the given fields of the thread's state and puts back what they held on the way out."""
    def __init__(self, **fields):
        self.fields = fields

    def __enter__(self):
        self.prev = {k: getattr(_STATE, k) for k in self.fields}
        _STATE.__dict__.update(self.fields)

    def __exit__(self, *exc):
        _STATE.__dict__.update(self.prev)


def scope(p, *, mx=None, bwd_split=None):
    """All of a `Precision`'s state at once (a model entry point); mx / bwd_split override the record's flag."""
    return _Scope(x3=p.x3, mx=p.mx if mx is None else bool(mx), bwd_split=p.bwd_split if bwd_split is None else bool(bwd_split))


def x3_mode(on=True):
    """Context manager: fp32 x fp32 contractions issued inside go through the bf16x3 split.  "full": "bf16x3"; "fwd" ("bf16x3f"):
    in the forward pass only, the backward contracts plain bf16 casts of the saved fp32 tensors; "x2" ("parity"): bf16x2 activations
    (hip_ops.X2), untagged fp32 operands still split.  Functions capture `x3_active()` in forward and act on it in backward."""
    return _Scope(x3=("full" if on is True else on) if on else False)


def mx_mode(on=True):
    """Context manager ("parity_mx"): inside the "x2" mode the big forward contractions -- the res4 / res5 convs, the box head's
    FC layers -- take the block-scaled f16mx kernels, and the tensors between them travel as unit-scale f16mx carriers."""
    return _Scope(mx=bool(on))


def backward_split(on=True):
    """Context manager ("parity_train"): Functions created inside keep the hi/lo split in their BACKWARD contractions too (three
    bf16 MFMA products on fp32 gradients, decoded bf16x2 activations and fp32 master weights) instead of plain bf16 products on
    the hi halves.  Which ones: WSOVOD_PT_SPLIT, default "dx" -- the input gradients carry the trajectory error; "dw,dx" is the
    "bf16x3" mode's backward ("The trained trajectory"; profiles/r06_parity_train_ablation.json)."""
    return _Scope(bwd_split=bool(on))


def x3_active():
    return _STATE.x3


def is_x2(x3):
    """`x3` (x3_active(), or what a Function captured of it) is the "parity" mode: activations are bf16x2 tensors (hip_ops.X2)."""
    return x3 == "x2"


def x2_active():
    return _STATE.x3 == "x2"


def mx_active():
    return bool(_STATE.mx) and x2_active()


def _bwd_split():
    """-> frozenset of {"dw", "dx"}: which backward contractions of a Function created now keep the split."""
    if not _STATE.bwd_split:
        return frozenset()
    which = os.environ.get("WSOVOD_PT_SPLIT", "dx")
    return frozenset(w for w in which.split(",") if w in ("dw", "dx"))


def _pt_dx():
    """WSOVOD_PT_DX: how a split input gradient dX = dA W is contracted under "parity_mx_train" -- "x2" (default): ONE bf16x2
    contraction on a masked gradient written as bf16x2 in one pass and the cached bf16x2 encoding of W^T; "x3": the
    generic route of "parity_train" (fp32 dA, a split pass, the fp32 master transposed and split at every step)."""
    return "x3" if os.environ.get("WSOVOD_PT_DX", "x2") == "x3" else "x2"


def _no_split(x3):
    """The x3 state a backward pass runs under: the forward-only modes ("fwd", "x2") contract in plain bf16."""
    return x3 if x3 not in ("fwd", "x2") else False
