"""The derived operand forms of a weight, cached on the tensor object: ONE attribute, one entry per format.

    bf16   compute-dtype copy of an fp32 master weight (functions.weight_shadow)
    x2     bf16x2 encoding (hip_ops.x2_cached)
    mx     f16mx (carrier, scales) (hip_ops.mx_cached), with the per-tensor scale byte of a trained weight
    x3     three-way bf16 split (hip_ops._split3_cached)
    x2t    bf16x2 encoding of the TRANSPOSE (hip_ops.x2t_cached): the "parity_mx_train" input gradient's B operand

An entry is (key, operand) with key = (version, data_ptr, view_rows_cols, variant); variant is the operand side of an x3
split, the dtype of a bf16 copy, else None.  Any in-place change of the tensor moves its version and the entry misses.

The update kernels write a parameter through raw pointers and refresh ONE of its operands in the same pass.  Python then
has to advance the version and re-stamp that entry: `refreshable` names the operand to hand to the kernel, `wrote` does the
bookkeeping after an eager launch, `replayed` after the replay of a captured step (no Python ran).  An operand that no
update kernel refreshes (x3, x2t) holds the values from BEFORE the update: it is never re-stamped, `wrote` and `replayed`
leave it to miss by version (x2t is also dropped there -- a whole weight's worth of bytes that nothing can read again).
Pure torch: the encoders stay with their kernels and are passed in.
"""
import torch

_ATTR = "_hip_operands"
_BF16 = torch.bfloat16
_bump = torch.autograd.graph.increment_version


class _Operands:
    __slots__ = ("bf16", "x2", "mx", "x3", "x2t", "mx_one_scale", "mx_byte")

    def __init__(self):
        self.bf16 = self.x2 = self.mx = self.x3 = self.x2t = self.mx_byte = None
        self.mx_one_scale = False  # the mx entry was encoded with ONE scale for the tensor (mx_byte): refreshable


def _operands(t):
    """The cache object of `t`, created at need; None for a tensor that refuses attributes (simply not cached)."""
    c = getattr(t, _ATTR, None)
    if c is None:
        c = _Operands()
        try:
            setattr(t, _ATTR, c)
        except AttributeError:
            return None
    return c


def current(t, fmt, view_rows_cols=None, variant=None):
    """The cached operand of `t` in format `fmt` if it matches the tensor as it stands, else None (nothing is encoded)."""
    e = getattr(getattr(t, _ATTR, None), fmt, None)
    if e is not None and e[0] == (t._version, t.data_ptr(), view_rows_cols, variant):
        return e[1]
    return None


def lookup(t, fmt, encode, view_rows_cols=None, variant=None, store=True, one_scale=False):
    """The operand of `t` in format `fmt`: the cached one if current, else encode(t.detach(), reshaped to view_rows_cols if
    given), stored unless `store` is False.  one_scale (mx): the encoder uses the ONE scale byte kept by `scale_byte`."""
    key = (t._version, t.data_ptr(), view_rows_cols, variant)
    c = getattr(t, _ATTR, None)
    e = getattr(c, fmt, None)
    if e is not None and e[0] == key:
        return e[1]
    src = t.detach()
    out = encode(src.reshape(view_rows_cols) if view_rows_cols is not None else src)
    if store:
        c = _operands(t)
        if c is not None:
            setattr(c, fmt, (key, out))
            if fmt == "mx":
                c.mx_one_scale = one_scale
    return out


def scale_byte(t, value=None):
    """The per-tensor scale byte (1-element device tensor) kept for `t`'s one-scale mx operand, or None.  With `value`: the
    first one is kept as it is, a later one is written into the kept tensor IN PLACE (captured step graphs and the
    optimizer's pointer table hold its address for the life of the parameter)."""
    c = getattr(t, _ATTR, None) if value is None else _operands(t)
    if c is None:
        return value
    if value is not None:
        if c.mx_byte is None:
            c.mx_byte = value
        else:
            c.mx_byte.copy_(value)
    return c.mx_byte


def one_scale_mx(t):
    """(carrier, scales) of `t`'s one-scale mx entry, current or stale (a full re-encode writes into them: their addresses
    are held like the byte's), else None."""
    c = getattr(t, _ATTR, None)
    return c.mx[1] if (c is not None and c.mx is not None and c.mx_one_scale) else None


def _refreshable(p, c):
    """(mx, x2, bf16) entries of `p` that are current AND of a form the update kernels can refresh: no view; mx with one
    scale for the tensor and its byte, mx / x2 with whole 32-element blocks; the copy in bfloat16.  Fourth: p.data_ptr()."""
    v, ptr = p._version, p.data_ptr()
    mx, x2, bf = c.mx, c.x2, c.bf16
    if mx is not None or x2 is not None:
        key = (v, ptr, None, None)
        if p.numel() % 32:
            mx = x2 = None
        if mx is not None and not (c.mx_one_scale and c.mx_byte is not None and mx[0] == key):
            mx = None
        if x2 is not None and x2[0] != key:
            x2 = None
    if bf is not None and bf[0] != (v, ptr, None, _BF16):
        bf = None
    return mx, x2, bf, ptr


def refreshable(p):
    """(format, operand) an update kernel takes as `shadow` for parameter `p`, (None, None) without one: the current one-scale
    f16mx operand as (carrier, scale byte), else the current bf16x2 operand, else the current bf16 copy.  Only this one is
    refreshed by the update; a second format goes stale by version and is re-encoded at its next use."""
    c = getattr(p, _ATTR, None)
    if c is None:
        return None, None
    mx, x2, bf, _ = _refreshable(p, c)
    if mx is not None:
        return "mx", (mx[1][0], c.mx_byte)
    if x2 is not None:
        return "x2", x2[1]
    if bf is not None:
        return "bf16", bf[1]
    return None, None


def wrote(p, fmt):
    """An update kernel wrote `p` through raw pointers and refreshed its `fmt` operand (as named by `refreshable`; None:
    none): the version advances, so that everything keyed on it is rebuilt, and that one entry is re-stamped."""
    _bump(p)
    c = getattr(p, _ATTR, None)
    if c is not None:
        c.x2t = None
    if fmt is not None:
        setattr(c, fmt, ((p._version, p.data_ptr(), None, _BF16 if fmt == "bf16" else None), getattr(c, fmt)[1]))


def replayed(p):
    """A replayed step graph wrote `p` (no Python ran, so `wrote` did not): the version advances and every refreshable entry
    that was current before the replay is re-stamped."""
    c = getattr(p, _ATTR, None)
    if c is None:
        _bump(p)
        return
    mx, x2, bf, ptr = _refreshable(p, c)
    _bump(p)
    c.x2t = None  # (encoded inside the graph from the weights before the update: stale, as after an eager step)
    if mx is not None:
        c.mx = ((p._version, ptr, None, None), mx[1])
    if x2 is not None:
        c.x2 = ((p._version, ptr, None, None), x2[1])
    if bf is not None:
        c.bf16 = ((p._version, ptr, None, _BF16), bf[1])
