"""-m gpu: the element-wise and head-support kernels (csrc/elementwise.hip, the data-aware head's backward and the MIL
kernels in csrc/heads.hip, format_rois in csrc/roi_pool.hip, im2col_rows in csrc/proposals.hip) against plain torch
restatements, at the shapes where their second code paths run: tails of the 8-elements-per-lane groups, unaligned
pointers and odd leading dimensions, clamped / masked branches, ties, empty segments, table splits.

Almost every kernel here rounds once, so most assertions are BIT equality with the torch expression (`same_bits`: NaN
payload and the sign of zero count).  Where a reduction is involved the bound is derived from its length, u = 2^-24:
a recursive fp32 sum of n terms is within n u of its sum of magnitudes (Higham, Accuracy and Stability, ch. 4: gamma_n
~ n u), whatever the order the lanes add in, plus one u for every further rounded operation.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.util import SENTINEL, bits, odd_view, outside_intact, same_bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F32, BF = torch.float32, torch.bfloat16
FLT_MIN = 1.17549435e-38  # fp32's smallest normal


def _ops():
    from wsovod_amd.layers import hip_ops as H

    return H


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _f32(v):
    """The fp32 value a Python float becomes when it is passed to a kernel as a `float` argument."""
    return torch.tensor(v, dtype=F32)


# ---------------------------------------------------------------------------------------------------------------------
# 1. row_l2norm_scale / row_l2norm_backward
# ---------------------------------------------------------------------------------------------------------------------
def _l2_rows(M, D, g):
    """Row kinds, rotated with M so that M = 1, 3, 4, 5 see different ones: 0 random, 1 all zero, 2 norm below eps,
    3 norm exactly 5 (or 3 when D == 1), 4 one huge element among small ones, 5 random with exact +0 / -0 entries."""
    x = torch.randn(M, D, generator=g)
    for r in range(M):
        kind = (r + M) % 6
        if kind == 1:
            x[r] = 0.0
        elif kind == 2:
            x[r] = 1e-14
        elif kind == 3:
            x[r] = 0.0
            x[r, 0] = 3.0
            if D > 1:
                x[r, D - 1] = 4.0
        elif kind == 4:
            x[r] *= 1e-3
            x[r, D // 2] = 1e15
        elif kind == 5:
            x[r, ::3] = 0.0
            x[r, 1::7] = -0.0
    return x


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [1, 63, 64, 65, 512, 768, 1000])
def test_row_l2norm_forward_and_backward(gpu, D, dtype):
    """scale = T / max(||z||, eps) and dz = d/dx [T relu(x) / max(||relu(x)||, eps)] . u (the kernel is handed z = relu(x),
    as the cosine head hands it; without relu_mask z = x keeps its negatives), against fp64 autograd on the STORED z.

    Forward: the sum of squares has D positive terms, each product rounded once, added in some order: relative error
    <= D u; the square root halves it and rounds once, the division rounds once, T and eps are rounded once each on their way
    into the kernel: (D + 8) u covers it.  Backward: z.u and ||z||^2 are two such sums (2 D u of sum |z u| / nn), then one
    quotient, one product, one difference, one product: (2 D + 8) u of s (|u| + |z| sum|z u| / nn)."""
    H = _ops()
    T, eps = 50.0, 1e-12
    eps32 = float(_f32(eps))
    for M in (1, 3, 4, 5, 1001):
        for relu in (False, True):
            g = _gen(1000 * D + 10 * M + int(relu))
            x = _l2_rows(M, D, g).to(dtype)
            z = torch.relu(x) if relu else x
            u = torch.randn(M, D, generator=g)
            zv, zbuf = odd_view((M, D), dtype, D + 3, 1, gpu)
            uv, ubuf = odd_view((M, D), F32, D + 5, 3, gpu)
            zv.copy_(z)
            uv.copy_(u)
            scale = H.row_l2norm_scale(zv, T, eps).cpu()
            dz = H.row_l2norm_backward(zv, uv, T, eps, relu_mask=relu).cpu()
            assert outside_intact(zbuf, zv) and outside_intact(ubuf, uv)
            tag = f"M={M} relu={relu}"

            xs = x.double().requires_grad_(True)
            zr = torch.relu(xs) if relu else xs
            nrm = zr.norm(dim=1, keepdim=True)
            (T * zr / nrm.clamp_min(eps32)).backward(u.double())
            want_dz = xs.grad
            assert bool(torch.isfinite(want_dz).all())
            nrm, zd, ud = nrm.detach(), zr.detach(), u.double()
            clamped = (nrm <= eps32).squeeze(1)
            assert not bool(((nrm > 0.5 * eps32) & (nrm < 2 * eps32)).any())  # no row near the branch point
            s = T / nrm.clamp_min(eps32)
            err = (scale.double() - s.squeeze(1)).abs() / s.squeeze(1)
            assert float(err.max()) <= (D + 8) * U, (tag, float(err.max()))
            proj = zd.abs() * (zd * ud).abs().sum(1, keepdim=True) / (nrm * nrm).clamp_min(1e-300)
            mag = s * (ud.abs() + torch.where(clamped[:, None], torch.zeros_like(proj), proj))
            berr = (dz.double() - want_dz).abs()
            assert bool((berr <= (2 * D + 8) * U * mag).all()), (tag, float((berr / mag.clamp_min(1e-300)).max()))
            # the clamped branch and the masked elements are single products / constants: exact
            active = (z.float() > 0) if relu else torch.ones(M, D, dtype=torch.bool)
            if bool(clamped.any()):
                want = torch.where(active, (_f32(T) / _f32(eps)) * u, torch.zeros(()))[clamped]
                assert same_bits(dz[clamped], want), tag
            assert bool((bits(dz)[~active] == 0).all()), tag
    # relu_mask with a z that was NOT produced by a ReLU: negatives, -0 and +0 are all "not active" -> exactly +0
    M = 9
    z = _l2_rows(M, D, _gen(D)).to(dtype)
    z[:, ::2] = -z[:, ::2].abs()
    z[0, :] = -0.0
    zv, _ = odd_view((M, D), dtype, D + 3, 1, gpu)
    zv.copy_(z)
    dz = H.row_l2norm_backward(zv, torch.randn(M, D, generator=_gen(D + 1)).to(gpu), T, eps, relu_mask=True).cpu()
    assert bool((bits(dz)[~(z.float() > 0)] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 2. scale_rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(1, 1), (3, 7), (5, 1204), (257, 512), (20, 768)])
def test_scale_rows(gpu, shape, out_dtype):
    H = _ops()
    R, Cc = shape
    g = _gen(R * 7 + Cc)
    x, s = torch.randn(R, Cc, generator=g), torch.randn(R, generator=g) * 3
    xv, xbuf = odd_view((R, Cc), F32, Cc + 3, 1, gpu)
    xv.copy_(x)
    out = torch.full((R + 2, Cc + 5), SENTINEL, dtype=out_dtype, device=gpu)
    H.scale_rows(xv, s.to(gpu), out)
    got = out.cpu()
    assert same_bits(got[:R, :Cc], (x * s[:, None]).to(out_dtype))
    fill = bits(torch.full((1,), SENTINEL, dtype=out_dtype))
    assert bool((bits(got[R:]) == fill).all()) and bool((bits(got[:, Cc:]) == fill).all())
    assert outside_intact(xbuf, xv)


# ---------------------------------------------------------------------------------------------------------------------
# 3. add_group_rows
# ---------------------------------------------------------------------------------------------------------------------
def _row_groups(M, g):
    """Groups 0..4 with 3 never used, repeats, and no order; neighbouring rows differ wherever M allows it."""
    rg = torch.tensor([4, 0, 0, 2, 1, 4, 2, 0, 1, 1, 4], dtype=torch.int32).repeat(M // 11 + 1)[:M].clone()
    if M > 64:
        pick = torch.randint(0, 4, (M - 64,), generator=g).to(torch.int32)
        rg[64:] = torch.where(pick == 3, torch.full_like(pick, 4), pick)
    return rg


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_add_group_rows(gpu, dtype, odd):
    H = _ops()
    for N in (1, 7, 8, 9, 20, 1204, 4096):
        for M in (1, 7, 8, 9, 1000):
            g = _gen(N * 31 + M)
            x = torch.randn(M, N, generator=g).to(dtype)
            add = torch.randn(5, N, generator=g)
            rg = _row_groups(M, g)
            if odd:
                xv, xbuf = odd_view((M, N), dtype, N + 3, 1, gpu)
                av, abuf = odd_view((5, N), F32, N + 1, 3, gpu)
                xv.copy_(x)
                av.copy_(add)
            else:
                xv, av = x.to(gpu), add.to(gpu)
            got = H.add_group_rows(xv, rg.to(gpu), av).cpu()
            want = (x.float() + add[rg.long()]).to(dtype)
            assert same_bits(got, want), (M, N)
            if odd:
                assert outside_intact(xbuf, xv) and outside_intact(abuf, av)


@pytest.mark.parametrize("shape", [(1, 32), (9, 64), (1000, 4096)])
def test_add_group_rows_x2_shapes(gpu, shape):
    """The bf16x2 form at the shapes test_gpu_bf16x2.py (77 x 96) lacks.  The sum is re-encoded as a (hi, lo) bf16 pair:
    16 significand bits, so the result is within 2^-16 of the fp32 sum (half an ulp of the pair), relative; near a
    cancellation the absolute bound is 2^-16 of the larger operand."""
    H = _ops()
    M, N = shape
    g = _gen(M + N)
    a, add, rg = torch.randn(M, N, generator=g), torch.randn(5, N, generator=g), _row_groups(M, g)
    ae = H.x2_encode(a.to(gpu))
    stored = H.x2_decode(ae).cpu()
    got = H.x2_decode(H.add_group_rows(ae, rg.to(gpu), add.to(gpu), x2=True)).cpu()
    want = stored.double() + add[rg.long()].double()
    bound = 2.0 ** -15 * torch.maximum(stored.abs(), add[rg.long()].abs()).double()  # two roundings: the sum, the pair
    assert bool(((got.double() - want).abs() <= bound).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. mask_transpose (wsovod_mask_transpose, _colsum, _ex through the one wrapper)
# ---------------------------------------------------------------------------------------------------------------------
def _mask_source(M, N, g, kind):
    """y with the values a `> 0` mask must get right: +0, -0, NaN, denormals of both signs."""
    y = torch.randn(M, N, generator=g)
    flat = y.view(-1)
    n = flat.numel()
    for k, v in enumerate((0.0, -0.0, float("nan"), 1e-40, -1e-40)):
        flat[k % n::13 + k] = v
    if n > 5:
        flat[:5] = torch.tensor([0.0, -0.0, float("nan"), 1e-40, -1e-40])
    return y.to(BF) if kind in ("bf16", "x2") else y


MT_COMBOS = [  # (dy dtype, y kind, out dtype)
    (F32, "same", F32), (F32, "same", BF), (BF, "same", BF), (BF, "same", F32),
    (F32, "bf16", F32), (F32, "bf16", BF), (F32, "x2", F32), (F32, "x2", BF),
    (F32, None, F32), (F32, None, BF), (BF, None, BF), (BF, None, F32),
]


@pytest.mark.parametrize("combo", MT_COMBOS, ids=lambda c: f"{str(c[0])[6:]}-{c[1]}-{str(c[2])[6:]}")
def test_mask_transpose(gpu, combo):
    H = _ops()
    dy_dtype, ykind, out_dtype = combo
    scale = 0.37
    shapes = [(1, 1), (65, 9), (150, 1204), (64, 64), (4096, 1024)]
    if ykind == "x2":  # the wrapper's contract: a bf16x2 y has whole 32-value groups
        shapes = [(1, 32), (65, 96), (64, 64), (4096, 1024)]
    for M, N in shapes:
        g = _gen(M * 5 + N)
        dy = torch.randn(M, N, generator=g).to(dy_dtype)
        if ykind is None:
            y_dev, active = None, torch.ones(M, N, dtype=torch.bool)
        else:
            y = _mask_source(M, N, g, ykind if ykind != "same" else ("bf16" if dy_dtype == BF else "f32"))
            if ykind == "x2":
                y_dev = H.x2_encode(y.float().to(gpu))
                hi = y_dev.view(BF).view(M, N // 32, 2, 32)[:, :, 0, :].reshape(M, N).cpu()  # the stored mask source
                active = hi.float() > 0
            else:
                yv, ybuf = odd_view((M, N), y.dtype, N + 7, 1, gpu)
                yv.copy_(y)
                y_dev, active = yv, y.float() > 0
            assert bool(active.any()) or M * N < 4
        masked = torch.where(active, dy.float() * _f32(scale), torch.zeros(()))  # fp32, before the output rounding
        want = masked.to(out_dtype)
        dyv, dybuf = odd_view((M, N), dy_dtype, N + 3, 1, gpu)
        dyv.copy_(dy)
        kw = dict(y_x2=ykind == "x2")
        big = M * N > 1 << 20
        tag = (M, N)

        # both outputs, default leading dimensions, contiguous dy
        dA, dAt = H.mask_transpose(dy.to(gpu), y_dev, scale, out_dtype, **kw)
        assert same_bits(dA.cpu(), want) and same_bits(dAt.cpu(), want.t().contiguous()), tag
        assert same_bits(dAt.cpu(), dA.cpu().t().contiguous()), tag
        # both outputs padded, unaligned dy, with the column sums
        ld_t, ld_p = (M + 7) // 8 * 8 + 8, N + 5
        cs = torch.zeros(N, device=gpu)
        dA, dAt = H.mask_transpose(dyv, y_dev, scale, out_dtype, ld_t=ld_t, ld_plain=ld_p, colsum=cs, **kw)
        dA, dAt, cs = dA.cpu(), dAt.cpu(), cs.clone().cpu()
        assert dA.shape == (M, ld_p) and dAt.shape == (N, ld_t)
        assert same_bits(dA[:, :N], want) and same_bits(dAt[:, :M], want.t().contiguous()), tag
        assert bool((bits(dA[:, N:]) == 0).all()) and bool((bits(dAt[:, M:]) == 0).all()), tag
        # column sums: M fp32 terms per column, added in a fixed order
        ref = masked.double().sum(0)
        mag = masked.double().abs().sum(0)
        assert bool(((cs.double() - ref).abs() <= M * U * mag).all()), (tag, float(((cs.double() - ref).abs() / mag.clamp_min(1e-300)).max()))
        pre = torch.randn(N, generator=g)
        cs2 = pre.clone().to(gpu)
        H.mask_transpose(dyv, y_dev, scale, out_dtype, want_plain=False, want_t=True, ld_t=ld_t, colsum=cs2, **kw)
        assert same_bits(cs2.cpu(), pre + cs), tag  # same bits twice, ADDED to what colsum held (one more fp32 addition)
        assert outside_intact(dybuf, dyv) and (y_dev is None or ykind == "x2" or outside_intact(ybuf, yv))
        if big:
            continue
        # each output alone; an odd ld_t (the transposed store's unaligned path)
        dA, none = H.mask_transpose(dyv, y_dev, scale, out_dtype, want_plain=True, want_t=False, **kw)
        assert none is None and same_bits(dA.cpu(), want), tag
        none, dAt = H.mask_transpose(dyv, y_dev, scale, out_dtype, want_plain=False, want_t=True, ld_t=M + 3, **kw)
        assert none is None and same_bits(dAt.cpu()[:, :M], want.t().contiguous()), tag
        assert bool((bits(dAt.cpu()[:, M:]) == 0).all()), tag
        # dA written in place into a view of a wider buffer
        ov, obuf = odd_view((M, N), out_dtype, N + 9, 3, gpu)
        dA, dAt = H.mask_transpose(dyv, y_dev, scale, out_dtype, out_plain=ov, want_plain=False, want_t=True, **kw)
        assert dA is ov and same_bits(ov.cpu(), want) and same_bits(dAt.cpu(), want.t().contiguous()), tag
        assert outside_intact(obuf, ov), tag


# ---------------------------------------------------------------------------------------------------------------------
# 5. transpose_cast, cast
# ---------------------------------------------------------------------------------------------------------------------
def _cast_specials():
    """fp32 values where an fp32 -> bf16 rounding can go wrong: round-to-nearest-even ties in both directions, +-Inf, NaN,
    -0, the largest value that still rounds to bf16's maximum, the tie above it (rounds to Inf), denormals."""
    raw = torch.tensor([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x7F7F7FFF, 0x7F7F8000, 0x00000001, 0x00008000],
                       dtype=torch.int32).view(F32)
    return torch.cat([raw, -raw, torch.tensor([float("inf"), float("-inf"), float("nan"), -0.0, 0.0, 1.0])])


def _to(x, dtype):
    """x.to(dtype), with IEEE 754's convertFormat for an fp32 NaN going to bf16: sign and leading payload kept, quieted
    (0x7fc00000 -> 0x7fc0, which is what the hardware conversion gives; torch's CPU conversion writes 0xffff instead)."""
    if not (x.dtype == F32 and dtype == BF):
        return x.to(dtype)
    x = x.contiguous()
    quiet = ((x.view(torch.int32) >> 16) | 0x40).to(torch.int16).view(BF)
    return torch.where(torch.isnan(x), quiet, x.to(BF))


def _with_specials(shape, g, dtype):
    x = torch.randn(shape, generator=g) * 4
    sp = _cast_specials()
    flat = x.view(-1)
    k = min(flat.numel(), sp.numel())
    flat[:k] = sp[:k]
    if flat.numel() > 3 * sp.numel():
        flat[-sp.numel():] = sp  # in the tail groups as well
    return x.to(dtype)


@pytest.mark.parametrize("dst_dtype", [F32, BF], ids=["to_f32", "to_bf16"])
@pytest.mark.parametrize("src_dtype", [F32, BF], ids=["f32", "bf16"])
def test_transpose_cast(gpu, src_dtype, dst_dtype):
    H = _ops()
    for R, Cc in ((1, 1), (7, 9), (8, 8), (64, 64), (65, 63), (130, 1204), (4096, 20)):
        g = _gen(R + 3 * Cc)
        x = _with_specials((R, Cc), g, src_dtype)
        want = _to(x.t().contiguous(), dst_dtype)
        xv, xbuf = odd_view((R, Cc), src_dtype, Cc + 3, 1, gpu)
        xv.copy_(x)
        assert same_bits(H.transpose_cast(x.to(gpu), dst_dtype).cpu(), want), (R, Cc)
        ld = (R + 7) // 8 * 8 + 8
        got = H.transpose_cast(xv, dst_dtype, ld_dst=ld).cpu()
        assert got.shape == (Cc, ld) and same_bits(got[:, :R], want) and bool((bits(got[:, R:]) == 0).all()), (R, Cc)
        ov, obuf = odd_view((Cc, R), dst_dtype, R + 5, 1, gpu)
        H.transpose_cast(xv, dst_dtype, out=ov)
        assert same_bits(ov.cpu(), want) and outside_intact(obuf, ov) and outside_intact(xbuf, xv), (R, Cc)


@pytest.mark.parametrize("dst_dtype", [F32, BF], ids=["to_f32", "to_bf16"])
@pytest.mark.parametrize("src_dtype", [F32, BF], ids=["f32", "bf16"])
def test_cast(gpu, src_dtype, dst_dtype):
    """(the wrapper makes its source contiguous: the contiguous form is what can be tested)"""
    H = _ops()
    for n in (1, 255, 256, 257, 2 ** 24 + 3):  # the last one is past the grid: the grid-stride loop
        x = _with_specials((n,), _gen(n), src_dtype)
        assert same_bits(H.cast(x.to(gpu), dst_dtype).cpu(), _to(x, dst_dtype)), n


# ---------------------------------------------------------------------------------------------------------------------
# 6. split3_bf16
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [0, 1])
def test_split3_bf16_tails_and_unaligned(gpu, side):
    """test_gpu_model_parity.py:142-164 pins 37 x 100 (contiguous and ld = 128, both 16-byte aligned) side by side and one
    stacked form; here: column tails around the 8-value group, an unaligned source, stacked padding for both sides."""
    H = _ops()
    for rows, cols in ((1, 1), (5, 7), (5, 8), (5, 9), (33, 1204)):
        g = _gen(rows + cols)
        x = torch.randn(rows, cols, generator=g) * torch.logspace(-3, 3, cols)[None]
        hi = x.to(BF)
        lo = (x - hi.float()).to(BF)
        blocks = (hi, lo, hi) if side else (hi, hi, lo)
        xv, xbuf = odd_view((rows, cols), F32, cols + 3, 1, gpu)
        xv.copy_(x)
        for src in (x.to(gpu), xv):
            cp = (cols + 7) // 8 * 8
            got = H.split3_bf16(src, side).cpu()
            assert got.shape == (rows, 3 * cp)
            for b, want in enumerate(blocks):
                assert same_bits(got[:, b * cp:b * cp + cols], want), (rows, cols, b)
                assert bool((bits(got[:, b * cp + cols:(b + 1) * cp]) == 0).all())
            rp = rows + 3
            st = H.split3_bf16(src, side, stack_rows=True, rows_pad=rp).cpu()
            assert st.shape == (3 * rp, cols)
            for b, want in enumerate(blocks):
                assert same_bits(st[b * rp:b * rp + rows], want), (rows, cols, b)
                assert bool((bits(st[b * rp + rows:(b + 1) * rp]) == 0).all())
        assert outside_intact(xbuf, xv)


# ---------------------------------------------------------------------------------------------------------------------
# 7. maxpool2x2_nhwc and its backward
# ---------------------------------------------------------------------------------------------------------------------
def _pool_rule(x, dout, stride, pad):
    """The documented backward restated: every window hands its gradient to its FIRST maximum in the scan order (0,0), (0,1),
    (1,0), (1,1) (strict '>'); the zero cells of the bottom / right padding take part and swallow their share.  An input
    position adds the windows it wins in the kernel's order (windows by ascending (ho, wo)).  -> (din, swallowed fp64)."""
    N, Hh, Ww, Cc = x.shape
    xp = F.pad(x, (0, 0, 0, 1, 0, 1)) if pad else x
    Ho, Wo = dout.shape[1:3]
    sl = lambda k: (slice(None), slice(k >> 1, (k >> 1) + stride * (Ho - 1) + 1, stride),
                    slice(k & 1, (k & 1) + stride * (Wo - 1) + 1, stride))
    best, arg = xp[sl(0)].clone(), torch.zeros((N, Ho, Wo, Cc), dtype=torch.long)
    for k in (1, 2, 3):
        upd = xp[sl(k)] > best
        best, arg = torch.where(upd, xp[sl(k)], best), torch.where(upd, torch.full_like(arg, k), arg)
    din = torch.zeros_like(xp)
    for k in (3, 2, 1, 0):  # position (h, w) is cell 3 of window (h-1, w-1), the first window the kernel visits
        din[sl(k)] += torch.where(arg == k, dout, torch.zeros(()))
    inner = din[:, :Hh, :Ww]
    return inner.contiguous(), float(din.double().sum() - inner.double().sum())


def _pool_inputs(shape, g):
    N, Hh, Ww, Cc = shape
    rnd = torch.randn(shape, generator=g)
    return {"random": rnd, "ties": torch.randint(-2, 3, shape, generator=g).float(),
            "negative": -rnd.abs() - 0.5, "constant": torch.full(shape, 1.5)}


POOL_FORMS = [(F32, False, 4), (F32, False, 8), (F32, False, 64), (BF, False, 8), (BF, False, 64), (F32, True, 32), (F32, True, 64)]


@pytest.mark.parametrize("form", POOL_FORMS, ids=lambda f: f"{'x2' if f[1] else str(f[0])[6:]}-C{f[2]}")
@pytest.mark.parametrize("hw", [(2, 2), (3, 3), (9, 11), (38, 50)])
def test_maxpool2x2_forward_and_backward(gpu, hw, form):
    """torch's CPU max_pool2d backward routes to the first maximum in the same scan order (checked here on the tie inputs as
    well: the restated rule and fp32 autograd agree), so both references are asserted."""
    H = _ops()
    dtype, x2, Cc = form
    Hh, Ww = hw
    N = 2
    for stride, pad in ((2, False), (1, True)):
        for name, x in _pool_inputs((N, Hh, Ww, Cc), _gen(Hh * Ww + Cc + stride)).items():
            tag = (stride, name)
            if x2:
                xd = H.x2_encode(x.view(-1, Cc).to(gpu)).view(N, Hh, Ww, Cc)
                xs = H.x2_decode(xd.view(-1, Cc)).view(N, Hh, Ww, Cc).cpu()  # the values the map really holds
            else:
                xs = x.to(dtype)
                xd = xs.to(gpu)
                xs = xs.float()
            nchw = xs.permute(0, 3, 1, 2).clone().requires_grad_(True)
            padded = F.pad(nchw, (0, 1, 0, 1)) if pad else nchw
            ref = F.max_pool2d(padded, 2, stride)
            want = ref.detach().permute(0, 2, 3, 1).contiguous()
            got = H.maxpool2x2_nhwc(xd, stride, zero_pad_br=pad, x2=x2)
            got = H.x2_decode(got.view(-1, Cc)).view(want.shape).cpu() if x2 else got.cpu()
            assert same_bits(got.float(), want), tag
            g = _gen(7)
            # dyadic gradients: every sum is exact, so the order of accumulation cannot hide or cause a difference
            dq = torch.randint(-8, 9, want.shape, generator=g).float() / 4
            din = H.maxpool2x2_nhwc_backward(xd, dq.to(gpu), stride, zero_pad_br=pad, x2=x2).cpu()
            rule, swallowed = _pool_rule(xs, dq, stride, pad)
            assert same_bits(din, rule), tag
            ref.backward(dq.permute(0, 3, 1, 2))
            assert torch.equal(din, nchw.grad.permute(0, 2, 3, 1)), tag  # torch's CPU rule is the documented one
            assert float(din.double().sum()) + swallowed == float(dq.double().sum()), tag
            if name == "negative" and pad:  # the zero pad wins the windows of the last row / column
                assert _pool_rule(xs, torch.ones_like(dq), stride, pad)[1] >= Hh + Ww - 1, tag
            # random normal gradients against the rule, added in the kernel's order
            dr = torch.randn(want.shape, generator=g)
            din = H.maxpool2x2_nhwc_backward(xd, dr.to(gpu), stride, zero_pad_br=pad, x2=x2).cpu()
            assert same_bits(din, _pool_rule(xs, dr, stride, pad)[0]), tag


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_maxpool2x2_keeps_the_number_beside_a_nan(gpu, dtype):
    """Decided: the pool is fmaxf, so a NaN cell loses to any number in its window and only an all-NaN window
    gives NaN -- the rule of the RoIPool scan (`v > maxval` skips NaN; test_gpu_roi_ops.py pins it); torch's max_pool2d
    would propagate the NaN instead."""
    H = _ops()
    nan = float("nan")
    x = torch.tensor([[1.0, nan, nan, nan], [-2.0, -3.0, nan, nan], [nan, 5.0, -1.0, nan], [4.0, nan, nan, -7.0]])
    x = x.view(1, 4, 4, 1).expand(1, 4, 4, 8).contiguous().to(dtype)
    got = H.maxpool2x2_nhwc(x.to(gpu), 2).cpu().float()
    assert torch.equal(got[0, :, :, 0][[0, 1, 1], [0, 0, 1]], torch.tensor([1.0, 5.0, -1.0]))
    assert bool(torch.isnan(got[0, 0, 1]).all())  # the all-NaN window
    got = H.maxpool2x2_nhwc(x.to(gpu), 1, zero_pad_br=True).cpu().float()
    assert not bool(torch.isnan(got[0, 3, :]).any()) and not bool(torch.isnan(got[0, :, 3]).any())  # the zero pad beside NaN
    assert float(got[0, 3, 3, 0]) == 0.0 and float(got[0, 0, 2, 0]) != float(got[0, 0, 2, 0])


def test_pgt_mine_and_label_refuses_more_classes_than_the_kernel_holds(gpu):
    """pgt_mine_label_kernel keeps min(classes of the image, 128) classes: the wrapper refuses the 129th instead of dropping
    it, from the host count when it is given, else from min(K, T), else by reading the offsets back."""
    H = _ops()
    K, M = 1203, 40
    g = _gen(3)
    scores = torch.rand(M, K, generator=g).to(gpu)
    xy = torch.rand(M, 2, generator=g) * 100
    boxes = torch.cat([xy, xy + 20 + torch.rand(M, 2, generator=g) * 50], 1).to(gpu)
    seg = torch.tensor([0, M], dtype=torch.int32, device=gpu)
    img = torch.rand(1, K, generator=g).to(gpu)

    def run(n_cls, **kw):
        cls = (torch.arange(n_cls, dtype=torch.int64) * 9).to(gpu)
        off = torch.tensor([0, n_cls], dtype=torch.int32, device=gpu)
        return H.pgt_mine_and_label(scores, boxes, seg, cls, off, img, K, 0.5, **kw)

    for kw in (dict(max_gt_per_image=129), dict()):
        with pytest.raises(RuntimeError, match="129 image-level GT classes"):
            run(129, **kw)
    for kw in (dict(max_gt_per_image=128), dict()):
        o = run(128, **kw)
        assert int(o["pgt_count"][0]) == 128 and bool((o["pgt_index"] >= 0).all())
        assert torch.equal(o["pgt_classes"].cpu(), torch.arange(128) * 9)
    # two images of 100 classes each: 200 in all, neither over the cap (decided by the read-back, or by the host count)
    cls = torch.cat([torch.arange(100), torch.arange(100) + 300]).to(gpu)
    off = torch.tensor([0, 100, 200], dtype=torch.int32, device=gpu)
    seg2 = torch.tensor([0, 25, M], dtype=torch.int32, device=gpu)
    o = H.pgt_mine_and_label(scores, boxes, seg2, cls, off, img.expand(2, K).contiguous(), K, 0.5)
    assert o["pgt_count"].cpu().tolist() == [100, 100]


# ---------------------------------------------------------------------------------------------------------------------
# 8. scale_by_device_scalar
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, (1 << 20) | 1])
def test_scale_by_device_scalar(gpu, n):
    """The kernel forms ONE quotient f = num / den (absent: 1) and multiplies every element by it."""
    H = _ops()
    x = torch.randn(n, generator=_gen(n))
    x[0] = 0.0
    one = torch.ones(())
    for num, den in ((3.7, None), (None, 3.7), (0.3, 7.0), (1.0, 0.0), (0.0, 0.0), (-2.0, 0.0)):
        tn = None if num is None else torch.tensor([num])
        td = None if den is None else torch.tensor([den])
        f = (one if tn is None else tn[0]) / (one if td is None else td[0])  # IEEE: x / 0 = +-Inf, 0 / 0 = NaN, no trap
        want = x * f
        got = H.scale_by_device_scalar(x.clone().to(gpu), None if tn is None else tn.to(gpu),
                                       None if td is None else td.to(gpu)).cpu()
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan), (num, den)  # (the payload of a generated NaN is the machine's choice)
        assert same_bits(got[~nan], want[~nan]), (num, den)
        if den == 0.0:
            assert not bool(torch.isfinite(got[1:]).any())


# ---------------------------------------------------------------------------------------------------------------------
# 9. sgd_momentum, sgd_momentum_multi
# ---------------------------------------------------------------------------------------------------------------------
MU = 0.9


def _sgd_reference_step(p, buf, g_scaled, lr, wd, first):
    """One torch.optim.SGD step in fp64 from the fp32 state (p, buf) the kernel started from -> (p64, buf64)."""
    q = p.double().clone().requires_grad_(True)
    opt = torch.optim.SGD([q], lr=lr, momentum=MU, weight_decay=wd)
    if not first:
        opt.state[q]["momentum_buffer"] = buf.double().clone()
    q.grad = g_scaled.double().clone()
    opt.step()
    return q.detach(), opt.state[q]["momentum_buffer"]


def _sgd_check(p0, b0, g_scaled, lr, wd, p1, b1, first, tag):
    """p: four fp32 operations per element (scale, decay, momentum, step), doubled: 8 u of the magnitudes involved."""
    pr, br = _sgd_reference_step(p0, b0, g_scaled, lr, wd, first)
    lr, wd = float(_f32(lr)), float(_f32(wd))
    m = g_scaled.double().abs() + wd * p0.double().abs() + MU * b0.double().abs()
    assert bool(((b1.double() - br).abs() <= 8 * U * m).all()), tag
    assert bool(((p1.double() - pr).abs() <= 8 * U * (p0.double().abs() + lr * m)).all()), tag


@pytest.mark.parametrize("numel", [1, 7, 4097, 300 * 70])
def test_sgd_momentum_single(gpu, numel):
    H = _ops()
    g = _gen(numel)
    p = torch.randn(numel, generator=g).to(gpu)
    buf = torch.zeros(numel, device=gpu)
    shadow = torch.full((numel,), SENTINEL, dtype=BF, device=gpu)
    lr, wd, gs = 0.02, 1e-4, 0.5
    for step in range(3):
        grad = torch.randn(numel, generator=g)
        p0, b0 = p.clone().cpu(), buf.clone().cpu()
        H.sgd_momentum(p, grad.to(gpu), buf, lr, MU, wd, grad_scale=gs, bf16_shadow=shadow)
        _sgd_check(p0, b0, grad * gs, lr, wd, p.cpu(), buf.cpu(), step == 0, (numel, step))
        assert same_bits(shadow.cpu(), p.cpu().to(BF))


SGD_SIZES = [1, 7, 4097, 300 * 70, 96 * 64, 32, 8195]


@pytest.mark.parametrize("count", [1, 32, 33, 65])
def test_sgd_momentum_multi(gpu, count):
    """Tables that fill one launch (32), spill by one (33) and span three (65); per-tensor lr / weight decay, fp32 and bf16
    gradients, bf16 / bf16x2 / no shadow, and tensors whose used_flag is 0 (left untouched bit for bit)."""
    H = _ops()
    g = _gen(count)
    gs = 0.5
    T = []
    for k in range(count):
        n = SGD_SIZES[(k + count) % len(SGD_SIZES)]
        t = dict(n=n, p=torch.randn(n, generator=g).to(gpu), buf=torch.zeros(n, device=gpu), lr=0.01 * (1 + k % 5),
                 wd=1e-4 * (k % 3), g_bf16=k % 2 == 1, unused=(count > 1 and k % 7 == 3) or k == 32)
        kind = k % 3 if n % 32 else (k % 2) * 2  # 0 none, 1 bf16, 2 bf16x2 (whole 32-value groups only)
        if kind == 2 and n % 32:
            kind = 1
        t["shadow"] = None if kind == 0 else torch.full((n,), SENTINEL, dtype=BF if kind == 1 else F32, device=gpu)
        t["flag"] = torch.tensor([0.0 if t["unused"] else 1.0], device=gpu)
        T.append(t)
    for step in range(3):
        entries, before = [], []
        for t in T:
            grad = torch.randn(t["n"], generator=g)
            grad = grad.to(BF) if t["g_bf16"] else grad
            t["grad"] = grad
            before.append((t["p"].clone().cpu(), t["buf"].clone().cpu(),
                           None if t["shadow"] is None else t["shadow"].clone().cpu()))
            entries.append((t["p"], grad.to(gpu), t["buf"], t["shadow"], t["lr"], t["wd"], t["flag"]))
        H.sgd_momentum_multi(entries, MU, grad_scale=gs)
        for k, (t, (p0, b0, s0)) in enumerate(zip(T, before)):
            p1, b1 = t["p"].cpu(), t["buf"].cpu()
            tag = (count, step, k, t["n"])
            if t["unused"]:
                assert same_bits(p1, p0) and same_bits(b1, b0), tag
                assert s0 is None or same_bits(t["shadow"].cpu(), s0), tag
                continue
            _sgd_check(p0, b0, t["grad"].float() * gs, t["lr"], t["wd"], p1, b1, step == 0, tag)
            if t["shadow"] is not None and t["shadow"].dtype == BF:
                assert same_bits(t["shadow"].cpu(), p1.to(BF)), tag
            elif t["shadow"] is not None:
                assert same_bits(t["shadow"].cpu().view(-1, 32), H.x2_encode(t["p"].view(-1, 32)).cpu()), tag


# ---------------------------------------------------------------------------------------------------------------------
# 10. pack_bf16_multi, sum_shards_bf16
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 32, 33])
def test_pack_bf16_multi(gpu, count):
    """Destinations are consecutive slices of one wire buffer, so odd sizes leave the later slices unaligned (scalar path)."""
    H = _ops()
    g = _gen(count)
    sizes = [(1, 8 * 1024 + 3, 7, 4096, 8, 4097)[(k + count) % 6] for k in range(count)]
    srcs = [_with_specials((n,), g, F32) for n in sizes]
    wire = torch.full((sum(sizes) + 16,), SENTINEL, dtype=BF, device=gpu)
    pairs, off = [], 0
    for s in srcs:
        pairs.append((s.to(gpu), wire[off:off + s.numel()]))
        off += s.numel()
    H.pack_bf16_multi(pairs)
    got = wire.cpu()
    assert same_bits(got[:off], _to(torch.cat(srcs), BF))
    assert bool((bits(got[off:]) == bits(torch.full((1,), SENTINEL, dtype=BF))).all())


@pytest.mark.parametrize("shards", [2, 3, 8])
def test_sum_shards_bf16(gpu, shards):
    H = _ops()
    for n in (8, 4096, 8 * 70001):
        src = (torch.randn(shards, n, generator=_gen(n + shards)) * 3).to(BF)
        acc = torch.zeros(n)
        for j in range(shards):  # fp32, in shard order
            acc = acc + src[j].float()
        dst = torch.full((n + 8,), SENTINEL, dtype=BF, device=gpu)
        H.sum_shards_bf16(src.view(-1).to(gpu), shards, dst[:n])
        got = dst.cpu()
        assert same_bits(got[:n], acc.to(BF)), n
        assert bool((bits(got[n:]) == bits(torch.full((1,), SENTINEL, dtype=BF))).all())
    # shards are whole 16-byte groups: any other size is refused, not run
    src = torch.zeros(shards * 12, dtype=BF, device=gpu)
    with pytest.raises(RuntimeError, match="whole 16-byte groups"):
        H.sum_shards_bf16(src, shards, torch.zeros(12, dtype=BF, device=gpu))


# ---------------------------------------------------------------------------------------------------------------------
# 11. data_aware_backward
# ---------------------------------------------------------------------------------------------------------------------
def _data_aware_case(N, Cc, Hd, P, Fd, g):
    """gap >= 0 (a global average of ReLU features).  Hidden unit j: every third has negative weights and bias (dead for
    every image, h1 exactly 0), the others positive ones (alive, far from the kink).  Prototype 0 saturates at +1, prototype 1
    at -1 (|pre-activation| > 20), the others stay inside tanh's bend.  With more than one image the last one's ddaf is
    zero."""
    gap = torch.rand(N, Cc, generator=g)
    W1 = torch.rand(Hd, Cc, generator=g) * (2.0 / Cc) + 1e-3
    b1 = torch.rand(Hd, generator=g) * 0.1 + 0.05
    dead = torch.arange(Hd) % 3 == 1
    W1[dead], b1[dead] = -W1[dead], -b1[dead]
    W2 = torch.randn(P, Hd, generator=g) * (1.0 / math.sqrt(Hd))
    b2 = torch.randn(P, generator=g) * 0.3
    b2[0] = 40.0
    if P > 1:
        b2[1] = -40.0
    E = torch.randn(P, Fd, generator=g)
    ddaf = torch.randn(N, Fd, generator=g)
    if N > 1:
        ddaf[N - 1] = 0.0
    return gap, W1, b1, W2, b2, E, ddaf, dead


def _data_aware_backward_from(gap, W2, E, ddaf, h1, h2):
    """The backward alone in fp64 from GIVEN h1, h2 (the fp32 forward's own, as the kernel is handed them): the formulas of
    data_aware_bwd_stage1 / stage2, and every gradient's sum of magnitudes (1 - t^2 taken as 1 + t^2)."""
    gap, W2, E, ddaf, h1, h2 = [t.double() for t in (gap, W2, E, ddaf, h1, h2)]
    live = (h1 > 0).double()
    dpre2 = (ddaf @ E.t()) * (1 - h2 * h2)
    dh1 = (dpre2 @ W2) * live
    grads = dict(dW1=dh1.t() @ gap, db1=dh1.sum(0), dW2=dpre2.t() @ h1, db2=dpre2.sum(0), dE=h2.t() @ ddaf)
    m_dpre2 = (ddaf.abs() @ E.abs().t()) * (1 + h2 * h2)
    m_dh1 = (m_dpre2 @ W2.abs()) * live
    mags = dict(dW1=m_dh1.t() @ gap.abs(), db1=m_dh1.sum(0), dW2=m_dpre2.t() @ h1.abs(), db2=m_dpre2.sum(0),
                dE=h2.abs().t() @ ddaf.abs())
    return grads, mags


def _data_aware_reference(gap, W1, b1, W2, b2, E, ddaf):
    """fp64 autograd through tanh(relu(g W1^T + b1) W2^T + b2) @ E, and the sum of magnitudes of every gradient: the same
    expressions with every factor replaced by its magnitude.  The kernel is handed the fp32 forward's h1 and h2, whose own
    rounding (a C-term dot, then an Hd-term dot: (C + Hd) u of the pre-activation's magnitude m_pre2) reaches the gradients
    through t = h2: |dt| <= (1 - t^2) |dpre2|, so |h2| carries (1 - t^2) m_pre2 besides itself and 1 - t^2 carries
    2 |t| (1 - t^2) m_pre2 besides 1 + t^2.  Saturated units (1 - t^2 = 0) carry none of it."""
    d = [t.double() for t in (gap, W1, b1, W2, b2, E, ddaf)]
    gap, W1, b1, W2, b2, E, ddaf = d
    for t in (W1, b1, W2, b2, E):
        t.requires_grad_(True)
    pre1 = gap @ W1.t() + b1
    h1 = torch.relu(pre1)
    pre2 = h1 @ W2.t() + b2
    h2 = torch.tanh(pre2)
    ((h2 @ E) * ddaf).sum().backward()
    grads = dict(dW1=W1.grad, db1=b1.grad, dW2=W2.grad, db2=b2.grad, dE=E.grad)
    with torch.no_grad():
        m_h1 = (gap.abs() @ W1.abs().t() + b1.abs()) * (h1 > 0)
        m_pre2 = m_h1 @ W2.abs().t() + b2.abs()
        sens = 1 - h2 * h2
        m_h2 = h2.abs() + sens * m_pre2
        m_dpre2 = (ddaf.abs() @ E.abs().t()) * ((1 + h2 * h2) + 2 * h2.abs() * sens * m_pre2)
        m_dh1 = (m_dpre2 @ W2.abs()) * (h1 > 0)
        mags = dict(dE=m_h2.t() @ ddaf.abs(), dW2=m_dpre2.t() @ m_h1, db2=m_dpre2.sum(0),
                    dW1=m_dh1.t() @ gap.abs(), db1=m_dh1.sum(0))
    return grads, mags, pre1.detach(), pre2.detach()


@pytest.mark.parametrize("dims", [(1, 512, 32, 5, 512), (3, 512, 32, 5, 4096), (32, 2048, 128, 5, 4096), (2, 48, 3, 7, 33)])
def test_data_aware_backward(gpu, dims):
    """Longest reduction chains, read off data_aware_bwd_stage1 / stage2: dE sums N images; dpre2 is an F-term dot, so dW2
    and db2 carry F + N; dh1 adds P terms to that, so dW1 and db1 carry F + P + N.  Every one of them also carries the C + Hd
    terms behind the h1 / h2 it is handed.  So two checks: (a) the backward KERNEL against the fp64 backward fed the same
    fp32 h1 / h2, at the bare (terms + 8) u of the sums of magnitudes -- the sharp one; (b) the whole head against fp64
    autograd that recomputes h1 and h2 itself, where the forward's own rounding counts: C + Hd more terms, and magnitudes
    that carry the sensitivity to h2 (_data_aware_reference)."""
    H = _ops()
    N, Cc, Hd, P, Fd = dims
    gap, W1, b1, W2, b2, E, ddaf, dead = _data_aware_case(N, Cc, Hd, P, Fd, _gen(sum(dims)))
    grads, mags, pre1, pre2 = _data_aware_reference(gap, W1, b1, W2, b2, E, ddaf)
    # the inputs do what they were arranged to do
    assert bool((pre1[:, dead] < -1e-3).all()) and bool((pre1[:, ~dead] > 1e-3).all())
    assert bool((pre2[:, 0] > 20).all()) and (P < 2 or bool((pre2[:, 1] < -20).all()))
    dev = [t.to(gpu) for t in (gap, W1, b1, W2, b2, E, ddaf)]
    _, h1, h2 = H.data_aware_forward(*dev[:6])
    assert bool((bits(h1.cpu()[:, dead]) == 0).all()) and bool((h1.cpu()[:, ~dead] > 0).all())
    got = H.data_aware_backward(dev[6], dev[0], dev[3], dev[5], h1, h2)
    again = H.data_aware_backward(dev[6], dev[0], dev[3], dev[5], h1, h2)
    chain = dict(dE=N, dW2=Fd + N, db2=Fd + N, dW1=Fd + P + N, db1=Fd + P + N)
    terms = {k: v + Cc + Hd for k, v in chain.items()}
    sharp, sharp_mags = _data_aware_backward_from(gap, W2, E, ddaf, h1.cpu(), h2.cpu())
    for name, a, b in zip(("dW1", "db1", "dW2", "db2", "dE"), got, again):
        assert same_bits(a.cpu(), b.cpu()), name  # same bits on every launch
        assert float(sharp_mags[name].max()) > 0 and float(mags[name].max()) > 0, name  # the case says something
        err = (a.cpu().double() - sharp[name]).abs()
        worst = float((err / sharp_mags[name].clamp_min(1e-300)).max())
        print(f"data_aware_backward {dims} {name} (given h1, h2): max err / magnitude = {worst:.3e}, bound {(chain[name] + 8) * U:.3e}")
        assert bool((err <= (chain[name] + 8) * U * sharp_mags[name]).all()), (name, worst)
        err = (a.cpu().double() - grads[name]).abs()
        bound = (terms[name] + 8) * U * mags[name]
        worst = float((err / mags[name].clamp_min(1e-300)).max())
        print(f"data_aware_backward {dims} {name}: max err / magnitude = {worst:.3e}, bound {(terms[name] + 8) * U:.3e}")
        assert bool((err <= bound).all()), (name, worst)
    assert bool((bits(got[0].cpu()[dead]) == 0).all()) and bool((bits(got[1].cpu()[dead]) == 0).all())  # dead units


# ---------------------------------------------------------------------------------------------------------------------
# 12. format_rois
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [[5], [1], [0, 1], [0, 5, 0, 0, 7, 1, 0], [3, 0, 4], [0, 0, 2, 0],
                                    [0, 30000, 0, 0, 1, 69998, 1, 0, 0]], ids=lambda c: f"G{len(c)}-M{sum(c)}")
def test_format_rois(gpu, counts):
    """Empty images first, in the middle, two in a row and last repeat an offset: the row's image is the LAST one that
    starts at or before it."""
    H = _ops()
    M, G = sum(counts), len(counts)
    g = _gen(M + G)
    boxes = torch.rand(M, 4, generator=g) * 500
    obj = torch.randn(M, generator=g)
    seg = torch.tensor([sum(counts[:i]) for i in range(G + 1)], dtype=torch.int32, device=gpu)
    img = torch.repeat_interleave(torch.arange(G), torch.tensor(counts))
    want = torch.cat([img.float()[:, None], boxes], 1)
    rois, scale = H.format_rois(boxes.to(gpu), seg, obj.to(gpu))
    assert same_bits(rois.cpu(), want) and same_bits(scale.cpu(), obj + 1.0)
    rois, scale = H.format_rois(boxes.to(gpu), seg)
    assert scale is None and same_bits(rois.cpu(), want)


# ---------------------------------------------------------------------------------------------------------------------
# 13. im2col_rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("Cc", [8, 64, 512])
def test_im2col_rows(gpu, Cc, dtype):
    H = _ops()
    N, Hh, Ww = 2, 7, 9
    g = _gen(Cc)
    x = torch.randn(N, Hh, Ww, Cc, generator=g).to(dtype)
    xd = x.to(gpu)
    for k in (1, 3):
        for stride in (1, 2):
            for pad in (0, 1, 2):
                for dil in (1, 2):
                    cols = F.unfold(x.float().permute(0, 3, 1, 2), k, dilation=dil, padding=pad, stride=stride)
                    L = cols.shape[-1]  # (N, C k k, L): channel-major, then tap
                    full = cols.view(N, Cc, k * k, L).permute(0, 3, 2, 1).reshape(N * L, k * k * Cc).to(dtype)
                    Ho = (Hh + 2 * pad - dil * (k - 1) - 1) // stride + 1
                    Wo = (Ww + 2 * pad - dil * (k - 1) - 1) // stride + 1
                    assert L == Ho * Wo
                    corners = [0, Wo - 1, (Ho - 1) * Wo, Ho * Wo - 1]
                    ids = torch.cat([torch.randperm(N * L, generator=g)[:40], torch.tensor(corners),
                                     torch.tensor(corners) + L, torch.tensor([-1, 5 % (N * L), 5 % (N * L), -7])])
                    got = H.im2col_rows(xd, ids.to(gpu), k, stride=stride, padding=pad, dilation=dil).cpu()
                    want = torch.where((ids >= 0)[:, None], full[ids.clamp_min(0)], torch.zeros((), dtype=dtype))
                    assert same_bits(got, want), (k, stride, pad, dil)


# ---------------------------------------------------------------------------------------------------------------------
# 14. the MIL head at numeric extremes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [-80.0, 80.0])
@pytest.mark.parametrize("K", [65, 1203])
def test_mil_extremes(gpu, K, shift):
    """Segments of 1, 0 and 5024 proposals in one launch; logits x 30 and shifted by +-80 so that most soft-max entries
    underflow; logits a view of a wider buffer.  Compared in the LOG domain: a row soft-max of K terms has a K-term sum (K u
    relative), the subtraction of the maximum, expf and the division each round once and the exponent's rounding enters the
    logarithm unscaled, together (K + 8) 2^-23.  The column soft-max Q is held to the same (K + 8) 2^-23, although its sum
    runs over the segment's R = 5024 proposals: 16 wavefronts add 314 terms each, then 16 partials, and that stays inside."""
    H = _ops()
    nums = [1, 0, 5024]
    M = sum(nums)
    g = _gen(K)
    logits = torch.randn(M, 2 * K, generator=g) * 30 + shift
    lv, lbuf = odd_view((M, 2 * K), F32, 2 * K + 3, 1, gpu)
    lv.copy_(logits)
    seg = torch.tensor([0, 1, 1, M], dtype=torch.int32, device=gpu)
    scores, P, Q = H.mil_forward(lv, seg, K)
    assert outside_intact(lbuf, lv)
    P, Q, scores = P.cpu(), Q.cpu(), scores.cpu()
    ld = logits.double()
    logP = torch.log_softmax(ld[:, :K], 1)
    logQ = torch.cat([torch.log_softmax(d, 0) for d in ld[:, K:].split(nums)])
    floor = math.log(FLT_MIN)
    for name, got, want, terms in (("P", P, logP, torch.full((M, 1), float(K))),
                                   ("Q", Q, logQ, torch.full((M, 1), float(K)))):
        normal = want > floor
        err = (torch.log(got.double().clamp_min(1e-300)) - want).abs()
        bound = ((terms + 8) * 2.0 ** -23).expand_as(err)
        print(f"mil K={K} shift={shift} {name}: max |dlog| / bound = {float((err / bound)[normal].max()):.3f}")
        assert bool((err <= bound)[normal].all()), name
        assert bool((got[~normal] < 2 * 1.18e-38).all()), name
    assert same_bits(scores, P * Q)
    for labels in (0.0, 1.0):  # all absent / all present
        y = torch.full((3, K), labels)
        loss, img, dS = H.image_bce_forward(scores.to(gpu), seg, y.to(gpu), float(3 * K))
        assert same_bits(img.cpu()[1], torch.full((K,), 1e-6)), labels  # the empty image: a clamped zero sum
        assert bool((dS.cpu()[1] == 0).all()), labels
        assert math.isfinite(float(loss)), labels
