"""GPU: the HIP conv backward of a trainable stage (wsovod_amd/modeling/conv_backward.py: `_masked`, `_conv_dgrad`, `_conv_wgrad`,
`_block_backward`, `_stage_backward_hip`, `_TrainableStem.backward`) against the linear fp64 reference of
tests/conv_backward_ref.py, block by block: BasicBlocks AND the BottleneckBlocks of the WSR_50 configs.

Every comparison is elementwise, |got - ref_as_read| <= c * u * B, no element exempt: u = 2^-24 (cd fp32) / 2^-9 (cd bf16), B the
reference evaluated over magnitudes, c counted from the code (conv_backward_ref.py: acc / c_dgrad / c_wgrad / c_block / c_stage,
each with its derivation; the numbers are repeated next to the cases below).  The reference takes ReLU masks and pool winners
from the HIP forward's own saved maps -- what the kernels are documented to do -- so nothing is excused for a flipped mask.
The observed max(err / (u * B)) of one run are kept in profiles/conv_backward_bounds.json (WSOVOD_CONV_BACKWARD_BOUNDS=<file>
writes them)."""
import json
import os

import pytest
import torch
from torch import nn

from tests import conv_backward_ref as R
from tests.util import same_bits

pytestmark = pytest.mark.gpu

# mode -> (the scope x3_mode(x3) of the forward, compute dtype of the backward)
MODES = {"fp32": (False, torch.float32), "bf16": (False, torch.bfloat16), "parity": ("x2", torch.bfloat16)}
GEOM = {"basic_identity": 0, "basic_projection": 1, "basic_pool_s2": 1, "basic_pool_s1": 0, "bottleneck_identity": 0,
        "bottleneck_dilated_projection": 1}
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _record_ratios():
    yield
    path = os.environ.get("WSOVOD_CONV_BACKWARD_BOUNDS")
    if path:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


def _H():
    from wsovod_amd.layers import hip_ops as H
    return H


def _encode(mode, x):
    """fp32 NHWC values on the GPU -> the mode's map format."""
    if mode == "fp32":
        return x.contiguous()
    if mode == "bf16":
        return x.to(torch.bfloat16).contiguous()
    return _H().x2_encode(x.reshape(-1, x.shape[-1]).contiguous()).view(x.shape)


def _values(t):
    """A map as the kernels left it (bf16 / fp32 / bf16x2 carrier, NHWC) -> its values, NCHW fp64 on the CPU."""
    from wsovod_amd.layers import carrier

    if carrier.fmt_of(t) == carrier.X2:
        t = _H().x2_decode(t.reshape(-1, t.shape[-1])).view(t.shape)
    return R.nchw64(t)


def _hi(t):
    """The hi halves of a bf16x2 carrier as stored (include/wsovod_hip.h: a row in groups of [32 hi | 32 lo] bf16 numbers) --
    the very numbers the weight-gradient kernel reads -- as NCHW fp64; None for any other map."""
    from wsovod_amd.layers import carrier

    if carrier.fmt_of(t) != carrier.X2:
        return None
    C = t.shape[-1]
    hi = t.detach().contiguous().view(torch.bfloat16).view(-1, C // 32, 2, 32)[:, :, 0, :].reshape(t.shape)
    return R.nchw64(hi)


def _check(name, got, ref, B, c, cd):
    """|got - ref| <= c * u * B on every element (an element without terms, B = 0, has to be 0)."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), name
    err, lim = (got - ref).abs(), R.U[cd] * B
    ratio = err / lim.clamp_min(1e-300)
    ratio[(lim == 0) & (err == 0)] = 0
    worst = float(ratio.max())
    RATIOS[name] = {"c": round(float(c), 6), "observed": round(worst, 6)}
    print(f"{name}: max err / (u * B) = {worst:.4g}, c = {float(c):.4g}")
    assert worst <= c, (name, worst, c)


def _randn(shape, seed, gpu):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32).to(gpu)


# ---- blocks: one forward and one reference per (kind, mode), shared by the tests ----------------------------------------------
_BLOCKS = {}


def _block_case(kind, mode, gpu):
    from wsovod_amd.modeling import conv_backward as BB

    if (kind, mode) not in _BLOCKS:
        H = _H()
        x3, cd = MODES[mode]
        block = R.make_block(kind).to(gpu)
        N, Hh, Ww = R.MAPS[GEOM[kind]]
        x = _encode(mode, _randn((N, Hh, Ww, block.in_channels), 11, gpu))
        with torch.no_grad(), H.x3_mode(x3):
            y, ins, out = BB._block_forward_saving(block, x)
        dy = _randn(tuple(y.shape), 12, gpu)
        ins64, out64, dy64 = [_values(t) for t in ins], _values(out), R.nchw64(dy)
        kw = dict(operand="as_read", cd=cd, x2=mode == "parity", ins_hi=[_hi(t) for t in ins] if mode == "parity" else None)
        ref = R.ref_block_backward(block, ins64, out64, dy64, True, **kw)
        bound = R.ref_block_backward(block, ins64, out64, dy64, True, absolute=True, **kw)
        _BLOCKS[(kind, mode)] = dict(block=block, x=x, y=y, ins=ins, out=out, dy=dy, ref=ref, bound=bound,
                                     c=R.c_block(block, N * Hh * Ww, cd))
    return _BLOCKS[(kind, mode)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", R.BLOCK_KINDS)
def test_the_recomputation_is_the_forward(gpu, kind, mode):
    """`_block_forward_saving` -- what the backward takes its masks from -- returns the bits of `block(x)`, also where the
    bf16 / bf16x2 forward of the stride-2 tail pool pools inside the 64-channel kernel and never writes the map."""
    H = _H()
    case = _block_case(kind, mode, gpu)
    with torch.no_grad(), H.x3_mode(MODES[mode][0]):
        y = case["block"](case["x"])
    assert same_bits(y, case["y"])
    if case["block"].has_pool:  # the saved full-resolution map pools to the forward's output
        with torch.no_grad(), H.x3_mode(MODES[mode][0]):
            assert same_bits(case["block"]._pool(case["out"]), y)


# c (conv_backward_ref.c_block), cd = bf16 [fp32: the accumulation term carries the bound].  A rounding to bf16 is 2^-8 = 2 u:
#   BasicBlock  64 ->  64  dx 4 + 2*576*2^-15 + 2^-15 = 4.035  [1155]   dW conv2 2.02   dW conv1 4.04
#   BasicBlock  64 -> 128  dx 4 + 2*1152*2^-15 + 2^-15 = 4.070 [2307]   dW conv2 2.02   dW conv1 4.07   dW shortcut 2.02
#   Bottleneck            dx 6 + 2*576*2^-15 + 2^-15 = 6.035  [1156]   dW conv3 2.02   dW conv2 4.02   dW conv1 6.04
#   (dW: 2 per rounding of the gradient -- once per conv it enters, this one included -- + 2*max(P, K of the convs behind)*2^-15
#   + 2^-15 for `dw * scale`; P = 198 / 273.  The first run had these at 1 / 3 / 5, a rounding counted as ONE u: the tail
#   conv's dW came out at 1.6 - 1.9 u B, under the 2 u of one bf16 rounding -- conv_backward_ref.ROUND.)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", R.BLOCK_KINDS)
def test_block_backward_against_fp64(gpu, kind, mode):
    from wsovod_amd.modeling import conv_backward as BB

    H = _H()
    case = _block_case(kind, mode, gpu)
    block, cd = case["block"], MODES[mode][1]
    convs = R.block_convs(block) + ([block.shortcut] if block.shortcut is not None else [])
    with torch.no_grad(), H.x3_mode(False):
        dx, grads = BB._block_backward(block, case["ins"], case["out"], case["dy"], cd, True)
        dx0, grads0 = BB._block_backward(block, case["ins"], case["out"], case["dy"], cd, False)
        convs[1].weight.requires_grad_(False)
        try:
            dx1, grads1 = BB._block_backward(block, case["ins"], case["out"], case["dy"], cd, True)
        finally:
            convs[1].weight.requires_grad_(True)
    torch.cuda.synchronize()
    (rx, rgrads), (bx, bgrads) = case["ref"], case["bound"]
    assert set(grads) == set(convs) and dx.dtype == torch.float32 and dx.shape == case["x"].shape
    _check(f"block/{kind}/{mode}/dx", dx.permute(0, 3, 1, 2), rx, bx, case["c"]["dx"], cd)
    for i, conv in enumerate(convs):
        assert grads[conv].dtype == torch.float32 and grads[conv].is_contiguous()
        _check(f"block/{kind}/{mode}/dW{i}", grads[conv], rgrads[conv], bgrads[conv], case["c"][conv], cd)
    # need_dx=False: no dx, the same weight gradients; a frozen conv: absent, everything else the same bits
    assert dx0 is None and set(grads0) == set(convs) and all(same_bits(grads0[c], grads[c]) for c in convs)
    assert set(grads1) == set(convs) - {convs[1]} and same_bits(dx1, dx) and all(same_bits(grads1[c], grads[c]) for c in grads1)


# ---- the single primitives: the reference gets the very operands the kernel reads, the accumulation term alone remains ---------
CONVS = {"k1_256_64": (1, 256, 64, 1), "k1_64_256": (1, 64, 256, 1), "k3_64_128": (3, 64, 128, 1), "k3d2_128_64": (3, 128, 64, 2),
         "k3d2_64_64": (3, 64, 64, 2)}  # (k, Cin, Cout, dilation)


def _conv(name, gpu):
    from wsovod_amd.modeling.backbone import Conv2d, FrozenBatchNorm2d, c2_msra_fill

    k, ci, co, d = CONVS[name]
    torch.manual_seed(300 + len(name) + ci + co)
    conv = Conv2d(ci, co, k, padding=d * (k - 1) // 2, dilation=d, bias=False, norm=FrozenBatchNorm2d(co))
    c2_msra_fill(conv)
    return R.seed_bn(conv, 400 + ci + co + k).to(gpu)


# c = 2 * K * 2^-24 / u, K = kh * kw * Cout the length of the one fp32 accumulation (conv_backward_ref.c_dgrad):
#   k1 256->64: K 64    k1 64->256: K 256    k3 64->128: K 1152    k3 dil 2 128->64 / 64->64: K 576
#   cd bf16: c = K * 2^-14 (0.004 .. 0.07; bf16 x bf16 products are exact in fp32)    cd fp32: c = 2 K
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(CONVS))
def test_conv_dgrad_against_fp64(gpu, name, mode):
    from wsovod_amd.modeling import conv_backward as BB

    H = _H()
    conv, cd = _conv(name, gpu), MODES[mode][1]
    N, Hh, Ww = R.MAPS[1 if mode == "parity" else 0]  # (bf16 and parity share cd: the second map under parity)
    g = _randn((N, Hh, Ww, conv.out_channels), 21, gpu).to(cd)
    with torch.no_grad(), H.x3_mode(False):
        dx = BB._conv_dgrad(g.view(-1, conv.out_channels), conv, N, Hh, Ww, cd)
    torch.cuda.synchronize()
    assert dx.dtype == torch.float32 and dx.shape == (N * Hh * Ww, conv.in_channels)
    g64 = R.nchw64(g)
    _check(f"dgrad/{name}/{mode}", dx.view(N, Hh, Ww, -1).permute(0, 3, 1, 2), R.ref_dgrad(g64, conv, cd),
           R.ref_dgrad(g64, conv, cd, absolute=True), R.c_dgrad(conv, cd), cd)


# c = (2 * P + 1) * 2^-24 / u (conv_backward_ref.c_wgrad): the one fp32 accumulation over the P patch rows -- the row blocks
# add into the same fp32 matrix -- and the fp32 multiply `dw * scale`.  P = 198: cd bf16 c = 0.0121, cd fp32 c = 397.
@pytest.mark.parametrize("blocked", [False, True], ids=["whole", "blocks_of_64"])
@pytest.mark.parametrize("fmt", list(MODES))
@pytest.mark.parametrize("name", list(CONVS))
def test_conv_wgrad_against_fp64(gpu, monkeypatch, name, fmt, blocked):
    from wsovod_amd.modeling import conv_backward as BB

    H = _H()
    conv, cd = _conv(name, gpu), MODES[fmt][1]
    k, ci, co, _ = CONVS[name]
    N, Hh, Ww = R.MAPS[0]  # P = 198: blocks of 64, 64, 64 and 6 rows; edges inside an image row and across the image boundary
    P = N * Hh * Ww
    xin = _encode(fmt, _randn((N, Hh, Ww, ci), 31, gpu))
    g = _randn((P, co), 32, gpu).to(cd)
    if blocked:
        monkeypatch.setattr(BB, "WGRAD_PATCH_BYTES", 64 * k * k * ci * xin.element_size())
        step = max(64, (BB.WGRAD_PATCH_BYTES // (k * k * ci * xin.element_size())) // 64 * 64)
        assert step == 64  # (a 1x1 conv reads the map itself and has no row blocks: it runs whole either way)
    with torch.no_grad(), H.x3_mode(False):
        dw = BB._conv_wgrad(g, xin, conv, cd)
    torch.cuda.synchronize()
    assert dw.dtype == torch.float32 and dw.shape == (co, ci, k, k) and dw.is_contiguous()
    g64, x64 = R.nchw64(g.view(N, Hh, Ww, co)), _values(xin)
    x2 = fmt == "parity"
    tag = f"wgrad/{name}/{fmt}/{'blocked' if blocked else 'whole'}"
    # (of a bf16x2 map the reference contracts the hi halves: meeting this bound IS being the hi-half gradient)
    hi = _hi(xin)
    _check(tag, dw, R.ref_wgrad(g64, x64, conv, cd, x2=x2, xhi=hi), R.ref_wgrad(g64, x64, conv, cd, x2=x2, xhi=hi, absolute=True),
           R.c_wgrad(P, cd), cd)
    if x2:
        # the documented grade against the unrounded map: one rounding of x to its hi half, 2^-9 of every term, + the
        # accumulation above; held to 2^-8 * B = 2 u B
        _check(tag + "/exact", dw, R.ref_wgrad(g64, x64, conv), R.ref_wgrad(g64, x64, conv, absolute=True), 2.0, cd)


# ---- `_TrainableStage` ---------------------------------------------------------------------------------------------------
STAGES = {"bottleneck": ("bottleneck_dilated_projection", "bottleneck_identity"), "basic_tail_pool": ("basic_identity", "basic_pool_s2")}


# c (conv_backward_ref.c_stage): a block's own c + the dx-c of every block behind it (cd bf16: Bottleneck 6.035, BasicBlock
# 4.035 per block; cd fp32: 1156 / 1155 per block); dx of the stage: the sum over its blocks, + one rounding (2 u) in "bf16" for
# `dx.to(x.dtype)`
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("stage_name", list(STAGES))
def test_trainable_stage_against_fp64(gpu, stage_name, mode):
    from wsovod_amd.modeling import conv_backward as BB

    H = _H()
    x3, cd = MODES[mode]
    blocks = [R.make_block(k, seed=i).to(gpu) for i, k in enumerate(STAGES[stage_name])]
    stage = nn.Sequential(*blocks)
    assert BB._hip_backward_ok(stage, x3)
    N, Hh, Ww = R.MAPS[1]
    x = _encode(mode, _randn((N, Hh, Ww, blocks[0].in_channels), 41, gpu))
    acts, Ps, cur = [], [], x
    with torch.no_grad(), H.x3_mode(x3):
        for b in blocks:
            nxt, ins, out = BB._block_forward_saving(b, cur)
            acts.append(([_values(t) for t in ins], _values(out), [_hi(t) for t in ins] if mode == "parity" else None))
            Ps.append(out.shape[0] * out.shape[1] * out.shape[2])
            cur = nxt
    frozen = blocks[0].conv2.weight
    frozen.requires_grad_(False)
    params = list(stage.parameters())
    dy = _randn(tuple(cur.shape), 42, gpu).to(cur.dtype)
    x.requires_grad_(True)
    y = BB._TrainableStage.apply(stage, x3, x, *params)
    assert same_bits(y.detach(), cur)
    y.backward(dy)
    torch.cuda.synchronize()
    kw = dict(operand="as_read", cd=cd, x2=mode == "parity")
    rx, rgrads = R.ref_stage_backward(blocks, acts, R.nchw64(dy), True, **kw)
    bx, bgrads = R.ref_stage_backward(blocks, acts, R.nchw64(dy), True, absolute=True, **kw)
    c = R.c_stage(blocks, Ps, cd)
    assert x.grad is not None and x.grad.dtype == (torch.float32 if mode == "parity" else x.dtype) and x.grad.shape == x.shape
    _check(f"stage/{stage_name}/{mode}/dx", x.grad.permute(0, 3, 1, 2), rx, bx, c["dx"] + (R.ROUND[cd] if mode == "bf16" else 0), cd)
    by_weight = {id(conv.weight): conv for conv in rgrads}
    assert frozen.grad is None and len(by_weight) == len(params) - 1
    for i, p in enumerate(params):  # parameter order: every gradient sits on its own parameter
        if p is frozen:
            continue
        conv = by_weight[id(p)]
        assert p.grad is not None and p.grad.shape == p.shape
        _check(f"stage/{stage_name}/{mode}/dW{i}", p.grad, rgrads[conv], bgrads[conv], c[conv], cd)
    # an input that takes no gradient: none is returned, the weight gradients are the same bits
    before = {id(p): p.grad.clone() for p in params if p.grad is not None}
    for p in params:
        p.grad = None
    x.requires_grad_(False)
    x.grad = None
    BB._TrainableStage.apply(stage, x3, x, *params).backward(dy)
    torch.cuda.synchronize()
    assert x.grad is None and frozen.grad is None
    assert all(same_bits(p.grad, before[id(p)]) for p in params if p is not frozen)


# ---- the stem ------------------------------------------------------------------------------------------------------------
# c, P = 2 * 16 * 20 = 640 rows, K of the 64-channel dgrads 576 (cd bf16; fp32 in brackets):
#   dW conv3  one rounding of the gradient (2 u) + (2*640 + 1) * 2^-15 = 2.04  [1282]
#   dW conv2  two = 4.04  [1283]
#   dW conv1  three = 6.04 + the patch operand: the kernel normalises the pixel in fp32 ((p - mean) / std on the fp32 mean and
#             std the reference takes too: 2 roundings, + 1 should it multiply by a rounded 1 / std) and rounds it to cd, the
#             reference rounds the fp64 value to cd: the two can land on neighbouring cd numbers, one spacing = two roundings
#             (4 u) -> 10.04 + 3 * 2^-15  [fp32: 1284 + 2 + 3]
@pytest.mark.parametrize("mode", ["fp32", "parity"])
def test_trainable_stem_against_fp64(gpu, mode):
    import torch.nn.functional as F
    from wsovod_amd.modeling import backbone as B, conv_backward as BB

    H = _H()
    x3, cd = MODES[mode]
    torch.manual_seed(500)
    stem = R.seed_bn(B.BasicStem(3, 64, norm="FrozenBN"), 501)
    net = B.ResNet(stem, [[R.make_block("basic_identity")]], freeze_at=0, precision=mode).to(gpu)
    img = torch.randint(0, 256, (2, 3, 32, 40), generator=torch.Generator().manual_seed(502), dtype=torch.uint8).to(gpu)
    sizes = torch.tensor([[32, 40], [32, 40]], dtype=torch.int32, device=gpu)
    mean, std = (103.53, 116.28, 123.675), (57.375, 57.12, 58.395)
    params = list(stem.parameters())
    assert [p.shape[1] for p in params] == [3, 64, 64]  # conv1, conv2, conv3
    out = BB._TrainableStem.apply(net, x3, img, sizes, mean, std, *params)
    dy = _randn(tuple(out.shape), 503, gpu)
    out.backward(dy)
    torch.cuda.synchronize()
    with torch.no_grad(), H.x3_mode(x3):
        a1 = net._stem_conv1(img, sizes, mean, std)
        a2 = B.hip_conv(a1, stem.conv2, relu=True)
        a3 = B.hip_conv(a2, stem.conv3, relu=True)
        assert same_bits(H.maxpool2x2_nhwc(a3, 2, x2=H.x2_active()), out.detach())
    h1, h2 = _hi(a1), _hi(a2)
    a1, a2, a3 = _values(a1), _values(a2), _values(a3)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).double().view(1, 3, 1, 1)
    pix = (img.cpu().double() - f32(mean)) / f32(std)
    pix = pix.to(cd).double()
    P = a3.shape[0] * a3.shape[2] * a3.shape[3]
    x2 = mode == "parity"
    refs = {}
    for absolute in (False, True):
        kw = dict(cd=cd, absolute=absolute)
        g = R.pool_backward(a3, R.nchw64(dy).abs() if absolute else R.nchw64(dy), 2) * (a3 > 0)
        dw3 = R.ref_wgrad(g, a2, stem.conv3, x2=x2, xhi=h2, **kw)
        g = R.ref_dgrad(g, stem.conv3, **kw) * (a2 > 0)
        dw2 = R.ref_wgrad(g, a1, stem.conv2, x2=x2, xhi=h1, **kw)
        g = R.ref_dgrad(g, stem.conv2, **kw) * (a1 > 0)
        cols = F.unfold(pix.abs() if absolute else pix, 3, padding=1, stride=2).permute(0, 2, 1).reshape(P, 27)
        scale = R.bn_scale(stem.conv1, cd)
        dw1 = (g.permute(0, 2, 3, 1).reshape(P, 64).t() @ cols).view(64, 3, 3, 3) * (scale.abs() if absolute else scale).view(-1, 1, 1, 1)
        refs[absolute] = (dw1, dw2, dw3)
    tail = R.acc(P, cd) + R.one_fp32(cd)
    rnd = R.ROUND[cd]
    cs = (3 * rnd + tail + 2 * rnd + 3 * R.one_fp32(cd), 2 * rnd + tail, rnd + tail)
    for i, p in enumerate(params):
        assert p.grad is not None and p.grad.shape == p.shape
        _check(f"stem/{mode}/dW conv{i + 1}", p.grad, refs[False][i], refs[True][i], cs[i], cd)
