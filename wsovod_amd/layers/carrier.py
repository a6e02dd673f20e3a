"""What the bytes of a float32-typed activation mean, recorded on the tensor object: ONE attribute, one tag.

In the "parity" / "parity_mx" precisions most activations are CARRIERS: torch.float32 tensors of the logical shape whose
4-byte slots hold no fp32 numbers but

    X2    interleaved bf16x2: (hi, lo) bf16 pairs in 32-value groups         (include/wsovod_hip.h: WSOVOD_BF16X2)
    X2P   planar bf16x2: the bf16 matrix of hi values, then the lo values    (WSOVOD_BF16X2P; the poolers, in training)
    MX    unit-scale f16mx: fp16 hi + two e4m3 planes per 32-value group     (WSOVOD_F16MX)

The format cannot be detected from the bytes.  A tag holds it (`fmt`) together with the plain bf16 rounding of the values
that travels with some carriers (`hi`: the operand of the next layer's weight gradient; of a planar carrier its first half,
no copy).  The kernel fronts that WRITE a carrier tag it (`tag`, the only place that sets the attribute); consumers ask
`fmt_of` / `hi_of`; a consumer that reads another format refuses (`refuse`).  A tensor that is not float32-typed is never a
carrier -- the bfloat16 view of a planar carrier's hi plane is a plain bf16 matrix.

Writers (kernel fronts in layers/hip_ops.py that tag their output): x2_encode / x2_encode_t, mx_encode(unit=True), mx_from_x2,
gemm_nt / gemm_mx with a carrier `out_dtype`, the RoI poolers, stem_conv1_x2 / stem_conv1_s1_x2 (X2), add_group_rows, and
maxpool2x2_nhwc (x2= -> X2; mx= -> MX: the f16mx pool copies the winner's fields, its output is a carrier of the same format).
Readers that take MX: gemm_mx, maxpool2x2_nhwc(mx=True), f16mx_to_f32, mx_range; everything else reads X2 / fp32 and refuses.

Which torch operations keep the tag (tests/test_carrier.py pins each):

    kept     whole views -- `view`, `flatten`, `reshape` of a contiguous tensor: `_base` is the tagged tensor, with the same
             data pointer and the same numel -- and the output of an autograd.Function tagged inside its forward
    dropped  slices (`_base` has another numel or pointer), `torch.cat`, `clone`, `detach`; a tensor that went through
             `ctx.save_for_backward` is to be taken as untagged (torch does not promise to hand the same object back)

Where model code makes such a tensor of a carrier and its bytes still are in the format -- a batch slice, the `cat` of the
parts, a re-wrapped saved tensor -- it says so with `like`.  Pure torch: importable without the HIP library.
"""
import torch

X2, X2P, MX = "bf16x2", "bf16x2p", "f16mx"
_ATTR = "_hip_carrier"


class _Tag:
    __slots__ = ("fmt", "hi")

    def __init__(self, fmt, hi):
        self.fmt, self.hi = fmt, hi


def tag(t, fmt, hi=None):
    """`t` was written in format `fmt` (with `hi` as its plain bf16 rounding) -> t.  A second tag replaces the first."""
    setattr(t, _ATTR, _Tag(fmt, hi))
    return t


def _tag_of(t):
    """The tag of `t`, or of the tensor `t` is a whole view of; None for anything that is not a float32-typed carrier."""
    if t is None or t.dtype != torch.float32:
        return None
    c = getattr(t, _ATTR, None)
    if c is None:
        b = getattr(t, "_base", None)
        if b is not None and b.data_ptr() == t.data_ptr() and b.numel() == t.numel():
            c = getattr(b, _ATTR, None)
    return c


def fmt_of(t):
    """X2, X2P or MX when `t` is a carrier, else None (real fp32 as far as anyone recorded, or another dtype)."""
    c = _tag_of(t)
    return c.fmt if c is not None else None


def hi_of(t):
    """The plain bf16 rounding attached to the carrier `t`, or None."""
    c = _tag_of(t)
    return c.hi if c is not None else None


def like(src, t):
    """`t` holds bytes of `src` in `src`'s format (a batch slice, a `cat` of such parts, a saved tensor wrapped again):
    tagged with that format -> t; untouched when `src` is no carrier.  `hi` belongs to the whole tensor and is not handed
    on, and a part of a planar carrier is not planar."""
    fmt = fmt_of(src)
    assert fmt != X2P, "a planar bf16x2 carrier is read whole"
    return tag(t, fmt) if fmt is not None else t


_REFUSAL = {
    X2P: "a PLANAR bf16x2 carrier where the interleaved layout is read (only the first FC layer's forward takes "
         "a_planar=True; x2_to_f32 decodes either layout)",
    MX: "an f16mx carrier where bf16x2 / fp32 values are read (f16mx operands go to gemm_mx)",
}


def refuse(who, tensors, reads=()):
    """A consumer of interleaved bf16x2 / real fp32 got `tensors` (None entries skipped): raises for one RECORDED as planar
    or f16mx instead of contracting its bytes.  `reads`: the formats among those two that this consumer does take (a declared
    planar operand), or does not refuse yet.  An X2 tag and no tag pass alike: consumers do not require a tag."""
    for t in tensors:
        fmt = fmt_of(t)
        if fmt in _REFUSAL and fmt not in reads:
            raise RuntimeError(f"wsovod_hip {who}: got {_REFUSAL[fmt]}")
