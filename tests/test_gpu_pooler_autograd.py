"""-m gpu: the autograd fronts of the poolers (wsovod_amd/layers/functions.py: `_RoIPool`, `_RoIAlign`, `_RoILoopPool`,
`_RoILoopPoolFused`) called as the model calls them -- `Fn.roi_pool(feat.requires_grad_(), ...)`, `out.backward(g)` -- against
the fp64 restatements of tests/functions_ref.py.

Forward: bit-exact against the C oracle (max pools), as the kernel tests require.
Backward, every element: |got - ref| <= (n_max + 1) 2^-24 B.  The kernel multiplies the output gradient by the roi's scale
(one rounding) and adds up to n_max such fp32 terms into a cell in arbitrary order (n_max - 1 roundings of partial sums no
larger than B); where B = 0 nothing is added and the result is exactly 0.  A bf16 map takes the fp32 gradient rounded to
bf16 at the end: one bf16 ulp of the reference on top.  RoIAlign: see `test_roi_align_autograd`.

The observed max(err / (2^-24 B)) of one run are kept in profiles/functions_autograd_bounds.json
(WSOVOD_FUNCTIONS_AUTOGRAD_BOUNDS=<file> writes them, merged per test id)."""
import pytest
import torch

from oracle import roi_ops as O
from tests import functions_ref as FR
from tests.util import same_bits

pytestmark = pytest.mark.gpu

N, Hh, Ww = FR.MAP
_ORACLE = {}


@pytest.fixture(scope="module", autouse=True)
def _record_ratios():
    yield
    FR.write_ratios()


def _fn():
    from wsovod_amd.layers import functions as Fn
    from wsovod_amd.layers import hip_ops as H
    return Fn, H


def _oracle(kind, C, dtype, size):
    """The C oracle's forward of the shared case: computed once per case and left unchanged."""
    key = (kind, C, dtype, size)
    if key not in _ORACLE:
        feat = FR.pooler_map(C, dtype, 100 + C, nonneg=kind == "loop")
        fwd = O.roi_loop_pool_forward if kind == "loop" else O.roi_pool_forward
        _ORACLE[key] = (feat,) + tuple(fwd(feat.float(), FR.pooler_rois(), FR.SCALE, size))
    return _ORACLE[key]


def _device_map(feat, cl, gpu):
    f = feat.to(gpu)
    if cl:
        f = f.contiguous(memory_format=torch.channels_last)
    return f.requires_grad_()


def _grad_like(out_shape, dtype, seed):
    """The gradient handed to out.backward: in the output's dtype, so its values are what the kernel reads."""
    return torch.randn(out_shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _check_backward(key, got, ref, B, c, dtype, extra=None):
    """|got - ref| <= c 2^-24 B (+ `extra`), every element; exactly 0 where B = 0 (and extra = 0); a bf16 map: + one bf16
    ulp of the reference (the Function's final cast)."""
    got = got.detach().cpu()
    assert got.dtype == dtype and got.shape == ref.shape
    bound = c * FR.U32 * B + (0 if extra is None else extra)
    zero = bound == 0
    assert bool(zero.any()) and bool((got[zero] == 0).all()), key
    err = (got.double() - ref).abs()
    if dtype == torch.bfloat16:
        err = (err - FR.bf16_ulp(ref) - 2.0 ** -8 * bound).clamp_min(0)  # (the rounded value's own ulp may be the next binade's)
    # (recorded: what the c term has to cover -- the error beyond `extra`, the fp32 sample coordinates' share)
    worst = FR.record(key, err if extra is None else (err - extra).clamp_min(0), FR.U32 * B)
    print(f"{key}: max err / (2^-24 B) = {worst:.3f}, c = {c}")
    assert bool((err <= bound).all()), (key, worst, c)
    assert float(ref.abs().max()) > 0.5, key  # the case says something


CASES = [(C, cl, dtype) for C in (8, 70) for cl in (False, True) for dtype in (torch.float32, torch.bfloat16)]
IDS = [f"C{C}-{'nhwc' if cl else 'nchw'}-{'bf16' if d == torch.bfloat16 else 'f32'}" for C, cl, d in CASES]


@pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("size", FR.POOL_SIZES, ids=["7x7", "3x5"])
@pytest.mark.parametrize("C,cl,dtype", CASES, ids=IDS)
def test_roi_pool_autograd(gpu, C, cl, dtype, size, scaled):
    Fn, H = _fn()
    feat, ref_out, ref_arg = _oracle("pool", C, dtype, size)
    rois, sc = FR.pooler_rois(), (FR.pooler_scale() if scaled else None)
    f = _device_map(feat, cl, gpu)
    out = Fn.roi_pool(f, rois.to(gpu), size, FR.SCALE, roi_scale=None if sc is None else sc.to(gpu))
    want = ref_out if sc is None else ref_out * sc.view(-1, 1, 1, 1)
    assert same_bits(out.detach().cpu(), want.to(dtype))
    _, arg = H.roi_pool_forward(f.detach(), rois.to(gpu), FR.SCALE, size)
    assert torch.equal(arg.cpu(), ref_arg)
    g = _grad_like(out.shape, dtype, 7)
    out.backward(g.to(gpu))
    ref, B, n_max = FR.roi_pool_backward(g, ref_arg, rois, sc, feat.shape)
    assert f.grad.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
    _check_backward(f"roi_pool-{C}-{cl}-{dtype}-{size}-{scaled}", f.grad, ref, B, n_max + 1, dtype)


@pytest.mark.parametrize("form", ["plain", "fused", "fused_scale"])
@pytest.mark.parametrize("size", FR.POOL_SIZES, ids=["7x7", "3x5"])
@pytest.mark.parametrize("C,cl,dtype", CASES, ids=IDS)
def test_roi_loop_pool_autograd(gpu, C, cl, dtype, size, form):
    """Both forms.  The reference scatters through the HIP forward's own argmax (asserted equal to the oracle's): row q of
    the (3R, ...) output is roi q mod R.  The fused form reads NHWC maps only: an NCHW map is refused, not converted."""
    Fn, H = _fn()
    feat, ref_out, ref_arg = _oracle("loop", C, dtype, size)
    rois = FR.pooler_rois()
    sc = FR.pooler_scale() if form == "fused_scale" else None
    f = _device_map(feat, cl, gpu)
    kw = {} if form == "plain" else dict(roi_scale=None if sc is None else sc.to(gpu), out_dtype=dtype)
    if form != "plain" and not cl:
        with pytest.raises(RuntimeError, match="NHWC"):
            Fn.roi_loop_pool(f, rois.to(gpu), size, FR.SCALE, **kw)
        return
    out = Fn.roi_loop_pool(f, rois.to(gpu), size, FR.SCALE, **kw)
    want = ref_out if sc is None else ref_out * sc.repeat(3).view(-1, 1, 1, 1)
    assert out.shape == (72, C) + size and same_bits(out.detach().cpu(), want.to(dtype))
    fwd = H.roi_loop_pool_forward if form == "plain" else H.roi_loop_pool_forward_fused
    _, arg = fwd(f.detach(), rois.to(gpu), FR.SCALE, size)
    assert torch.equal(arg.cpu(), ref_arg)
    g = _grad_like(out.shape, dtype, 8)
    out.backward(g.to(gpu))
    ref, B, n_max = FR.loop_pool_backward(g, arg, rois, sc, feat.shape)
    _check_backward(f"roi_loop_pool-{form}-{C}-{cl}-{dtype}-{size}", f.grad, ref, B, n_max + 1, dtype)


@pytest.mark.parametrize("fmt", ["X2", "MX"])
def test_fused_loop_pool_backward_ignores_the_output_encoding(gpu, fmt):
    """out_dtype bf16x2 under the "parity" scope and f16mx under "parity_mx" (the kernel writes carriers only for NHWC maps
    with a multiple of 256 channels and 7 bins across: C = 256): the same `g` gives the gradient of the fp32-output run bit
    for bit -- the argmax does not depend on the encoding, the backward does not read the output.  The scatter adds with
    atomics in no fixed order: a sum of up to two fp32 terms has the same bits in any order, so "bit for bit" is asserted on
    the cells that receive at most two; the others (three terms and more) are held to the fp32 bound of both runs."""
    Fn, H = _fn()
    from wsovod_amd.layers import precision

    feat = FR.pooler_map(256, torch.float32, 9, nonneg=True)
    rois, sc = FR.pooler_rois(), FR.pooler_scale()
    g = _grad_like((72, 256, 7, 7), torch.float32, 10).to(gpu)
    grads, args = {}, {}
    for name, scope, od in (("f32", None, torch.float32),
                            (fmt, precision.scope(precision.TABLE["parity" if fmt == "X2" else "parity_mx"]), getattr(H, fmt))):
        f = _device_map(feat, True, gpu)
        with (scope if scope is not None else precision.x3_mode(False)):
            out = Fn.roi_loop_pool(f, rois.to(gpu), (7, 7), FR.SCALE, roi_scale=sc.to(gpu), out_dtype=od)
            _, args[name] = H.roi_loop_pool_forward_fused(f.detach(), rois.to(gpu), FR.SCALE, (7, 7), roi_scale=sc.to(gpu),
                                                          out_dtype=od)
        assert od == torch.float32 or H.carrier.fmt_of(out) == od
        out.backward(g)
        grads[name] = f.grad.cpu()
    assert torch.equal(args["f32"], args[fmt])
    ref, B, n_max = FR.loop_pool_backward(g, args["f32"], rois, sc, feat.shape)
    cnt = FR.pool_scatter(torch.ones(72, 256, 7, 7), args["f32"], rois[:, 0].repeat(3), None, feat.shape)[0]
    few = cnt <= 2
    print(f"carrier {fmt}: {int(few.sum())} of {few.numel()} cells take <= 2 terms; whole gradient equal: "
          f"{same_bits(grads['f32'], grads[fmt])}")
    assert int((cnt == 2).sum()) > 100 and same_bits(grads["f32"][few], grads[fmt][few])
    for name in ("f32", fmt):
        _check_backward(f"roi_loop_pool-carrier-{name}", grads[name], ref, B, n_max + 1, torch.float32)


@pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("aligned,sampling_ratio", [(True, 0), (False, 2), (True, 2), (False, 0)])
@pytest.mark.parametrize("size", FR.POOL_SIZES, ids=["7x7", "3x5"])
@pytest.mark.parametrize("C,cl,dtype", [(8, False, torch.float32), (70, True, torch.float32), (70, False, torch.bfloat16),
                                        (8, True, torch.bfloat16)], ids=["C8-nchw-f32", "C70-nhwc-f32", "C70-nchw-bf16", "C8-nhwc-bf16"])
def test_roi_align_autograd(gpu, C, cl, dtype, size, aligned, sampling_ratio, scaled):
    """`roi_align_bwd`: per output element g = grad * inv_count (1 rounding), * scale (1), then per sample four atomic adds of
    g * w (1 each, the weight itself a product of two fp32 differences).  A cell that receives n_max adds: n_max - 1
    roundings of partial sums: c = n_max + 3 on B = the scatter of |grad * scale| * w / count.  The weights come from sample
    coordinates the kernel computes in fp32 (at most delta off, functions_ref._align_rois): each weight moves by at most
    3 delta, on the sample's own cells or -- across a cell border -- their neighbours: + 3 D (functions_ref.roi_align_backward).
    n_max is counted over the same reach.  Forward: the same two terms on sum w |feat| / count: every sample adds four
    products to the running sum (4 roundings per sample, `count` samples), then the two scalings and the output's own
    rounding: c = 4 * count + 3 with the largest sample count of the case."""
    Fn, H = _fn()
    feat = FR.pooler_map(C, dtype, 200 + C)
    rois, sc = FR.pooler_rois(), (FR.pooler_scale() if scaled else None)
    assert FR.roi_align_margin(rois, FR.SCALE, size, sampling_ratio, aligned, Hh, Ww) > 1e-3
    f = _device_map(feat, cl, gpu)
    out = Fn.roi_align(f, rois.to(gpu), size, FR.SCALE, sampling_ratio, aligned, roi_scale=None if sc is None else sc.to(gpu))
    assert out.dtype == dtype
    s = torch.ones(24, dtype=torch.float64) if sc is None else sc.double()
    ref_out = FR.roi_align(feat.double(), rois, FR.SCALE, size, sampling_ratio, aligned) * s.view(-1, 1, 1, 1)
    mag = FR.roi_align(feat.double().abs(), rois, FR.SCALE, size, sampling_ratio, aligned) * s.view(-1, 1, 1, 1)
    decoded = FR._align_rois(rois, FR.SCALE, size, sampling_ratio, aligned, Hh, Ww)
    delta, count = max(d for *_, d in decoded), max(round(1.0 / inv) for _, inv, *_ in decoded)
    tol = (4 * count + 3) * FR.U32 * mag + 4 * 3 * delta * float(feat.float().abs().max()) * s.view(-1, 1, 1, 1) * (mag > 0)
    err = (out.detach().cpu().double() - ref_out).abs()
    if dtype == torch.bfloat16:
        err = (err - FR.bf16_ulp(ref_out) - 2.0 ** -8 * tol).clamp_min(0)
    assert bool((err <= tol).all()), float((err - tol).max())
    g = _grad_like(out.shape, dtype, 11)
    out.backward(g.to(gpu))
    ref, B, D, n_max = FR.roi_align_backward(g, rois, sc, FR.SCALE, sampling_ratio, aligned, feat.shape)
    _check_backward(f"roi_align-{C}-{cl}-{dtype}-{size}-{aligned}-{sampling_ratio}-{scaled}", f.grad, ref, B, n_max + 3, dtype,
                    extra=3 * D)
