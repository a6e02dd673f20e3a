"""-m gpu: wsovod_roi_loop_pool_forward_ex, the three-output pool with the objectness scale and the output encoding fused.

Expected values come from the existing fp32 entry: `H.roi_loop_pool_forward(...)[0] * roi_scale.repeat(3)[:, None, None, None]`
in fp32 torch arithmetic -- the sequence the ROI heads ran before the fused entry existed.  Every output format of the fused
entry must hold exactly those fp32 values in its own encoding: fp32 bit for bit, bf16 as torch casts, bf16x2 (interleaved,
planar, and the plain bf16 copy) as torch's hi = v.bfloat16(), lo = (v - hi).bfloat16() in the documented layout and as the
repo's own bf16x2 encoder writes them, f16mx as the repo's unit-scale f16mx encoder writes them."""
import pytest
import torch

from tests.util import same_bits

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SCALE = 1.0 / 8.0
N_IMG, MAP_H, MAP_W = 2, 19, 25  # a 152 x 200 image at stride 8
R = 23


def _boxes():
    """(23, 5) pooler-format rois: 22 boxes on image 0 -- 16 random ones and the six edge cases -- and a single box on
    image 1."""
    g = torch.Generator().manual_seed(5)
    x1 = torch.rand(16, generator=g) * 150
    y1 = torch.rand(16, generator=g) * 110
    w = torch.rand(16, generator=g) * 120 + 4
    h = torch.rand(16, generator=g) * 90 + 4
    rnd = torch.stack([x1, y1, (x1 + w).clamp(max=199.0), (y1 + h).clamp(max=151.0)], dim=1)
    edge = torch.tensor([
        [50.0, 40.0, 50.0, 40.0],        # degenerate: zero area
        [64.0, 48.0, 65.0, 49.0],        # one pixel
        [400.0, 300.0, 500.0, 380.0],    # wholly outside the image (beyond the map on both axes)
        [2.0, 3.0, 60.0, 50.0],          # the grown context rectangle is clipped at the left and the top border
        [80.0, 64.0, 82.0, 66.0],        # the shrunk rectangle rounds to the box itself: the frame has no hole
        [120.0, 90.0, 199.0, 151.0],     # (the grown rectangle clipped at the right and the bottom border)
    ])
    img0 = torch.cat([rnd, edge])
    rois0 = torch.cat([torch.zeros(len(img0), 1), img0], dim=1)
    rois1 = torch.tensor([[1.0, 30.0, 20.0, 150.0, 120.0]])  # image 1 holds a single box
    rois = torch.cat([rois0, rois1])
    assert rois.shape == (R, 5)
    return rois


def _case(gpu, dtype, C):
    g = torch.Generator().manual_seed(C + (1 if dtype == BF else 0))
    feat = torch.relu(torch.randn(N_IMG, C, MAP_H, MAP_W, generator=g)).to(dtype)  # post-ReLU: about half exact zeros
    assert bool((feat == 0).any())
    f = feat.to(gpu).contiguous(memory_format=torch.channels_last)
    rois = _boxes().to(gpu)
    sc = (torch.rand(R, generator=g) * 1.5 + 0.25).to(gpu)
    return f, rois, sc


def _x2_planes(t, rows, cols):
    """(hi, lo) bf16 matrices of an interleaved bf16x2 carrier: per 32-value group 32 hi values, then 32 lo values."""
    raw = t.contiguous().view(BF).view(rows, cols // 32, 2, 32)
    return raw[:, :, 0, :].reshape(rows, cols), raw[:, :, 1, :].reshape(rows, cols)


@pytest.mark.parametrize("size", [(7, 7), (3, 7)], ids=["7x7", "3x7"])
@pytest.mark.parametrize("C", [256, 512])
@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16map", "fp32map"])
def test_fused_outputs_hold_the_scaled_fp32_values_in_every_format(gpu, monkeypatch, dtype, C, size):
    from wsovod_amd.layers import hip_ops as H

    f, rois, sc = _case(gpu, dtype, C)
    base, base_arg = H.roi_loop_pool_forward(f, rois, SCALE, size)
    want = base * sc.repeat(3)[:, None, None, None]  # fp32, torch
    rows, cols = 3 * R, C * size[0] * size[1]
    want2d = want.view(rows, cols)
    hi = want2d.bfloat16()
    lo = (want2d - hi.float()).bfloat16()
    # the edge cases are what they claim to be: an empty region for the outside box, frame == region without a hole
    assert float(base[18].abs().max()) == 0.0 and float(base[R + 18].abs().max()) == 0.0
    assert torch.equal(base[R + 20], base[20])
    assert not torch.equal(base[R:2 * R], base[:R]) and not torch.equal(base[2 * R:], base[:R])

    # fp32, with and without argmax
    o32, arg = H.roi_loop_pool_forward_fused(f, rois, SCALE, size, roi_scale=sc, out_dtype=torch.float32, need_argmax=True)
    assert same_bits(o32.cpu(), want.cpu()) and torch.equal(arg, base_arg)
    o32n, none = H.roi_loop_pool_forward_fused(f, rois, SCALE, size, roi_scale=sc, out_dtype=torch.float32, need_argmax=False)
    assert none is None and same_bits(o32n.cpu(), o32.cpu())
    # without a scale: the existing entry's values
    plain, _ = H.roi_loop_pool_forward_fused(f, rois, SCALE, size, out_dtype=torch.float32, need_argmax=False)
    assert same_bits(plain.cpu(), base.cpu())
    # bf16
    for am in (True, False):
        ob, arg = H.roi_loop_pool_forward_fused(f, rois, SCALE, size, roi_scale=sc, out_dtype=BF, need_argmax=am)
        assert ob.dtype == BF and same_bits(ob.cpu(), want.bfloat16().cpu())
        assert (arg is None) if not am else torch.equal(arg, base_arg)
    # interleaved bf16x2, no copy
    ox, _ = H.roi_loop_pool_forward_fused(f, rois, SCALE, size, roi_scale=sc, out_dtype=H.X2, need_argmax=False)
    assert H.carrier.fmt_of(ox) == H.X2 and H.x2_hi_pop(ox) is None and ox.shape == want.shape
    ghi, glo = _x2_planes(ox, rows, cols)
    assert same_bits(ghi.cpu(), hi.cpu()) and same_bits(glo.cpu(), lo.cpu())
    assert torch.equal(ox.view(rows, cols).view(torch.int32), H.x2_encode(want2d.contiguous()).view(torch.int32))
    # planar bf16x2: the training form -- hi plane of all 3R rows, then the lo plane; the copy IS the hi plane
    op, arg = H.roi_loop_pool_forward_fused(f, rois, SCALE, size, roi_scale=sc, out_dtype=H.X2, need_argmax=True, want_hi=True)
    assert H.x2_planar_of(op) and torch.equal(arg, base_arg)
    flat = op.view(-1).view(BF)
    assert same_bits(flat[:rows * cols].view(rows, cols).cpu(), hi.cpu())
    assert same_bits(flat[rows * cols:].view(rows, cols).cpu(), lo.cpu())
    php = H.x2_hi_pop(op)
    assert php is not None and php.data_ptr() == op.data_ptr() and php.dtype == BF and php.shape == op.shape
    # interleaved bf16x2 + the plain bf16 copy (the form of steps too large for the planar one)
    monkeypatch.setattr(H, "X2_PLANAR", False)
    oc, _ = H.roi_loop_pool_forward_fused(f, rois, SCALE, size, roi_scale=sc, out_dtype=H.X2, need_argmax=False, want_hi=True)
    monkeypatch.undo()
    assert H.carrier.fmt_of(oc) == H.X2 and torch.equal(oc.view(torch.int32), ox.view(torch.int32))
    assert same_bits(H.x2_hi_pop(oc).view(rows, cols).cpu(), hi.cpu())
    # unit-scale f16mx: the bytes of the repo's encoder on the same fp32 values; its bf16 copy
    enc = H.mx_encode(want2d.contiguous(), unit=True)[0]
    for want_hi in (False, True):
        om, _ = H.roi_loop_pool_forward_fused(f, rois, SCALE, size, roi_scale=sc, out_dtype=H.MX, need_argmax=False,
                                              want_hi=want_hi)
        assert H.mx_of(om) and om.shape == want.shape
        assert torch.equal(om.view(rows, cols).view(torch.int32), enc.view(torch.int32))
        cp = H.x2_hi_pop(om)
        assert (cp is None) if not want_hi else same_bits(cp.view(rows, cols).cpu(), hi.cpu())


def test_no_rois_returns_empty_tensors(gpu):
    from wsovod_amd._lib import profile_collect, profile_enable, profile_reset
    from wsovod_amd.layers import hip_ops as H

    f, rois, sc = _case(gpu, BF, 256)
    profile_enable(True)
    try:
        profile_reset()
        for fmt in (torch.float32, BF, H.X2, H.MX):
            out, arg = H.roi_loop_pool_forward_fused(f, rois[:0], SCALE, (7, 7), roi_scale=sc[:0], out_dtype=fmt,
                                                     need_argmax=True, want_hi=True)
            assert out.shape == (0, 256, 7, 7) and arg.shape == (0, 256, 7, 7) and arg.dtype == torch.int32
        torch.cuda.synchronize()
        launched = [e for e in profile_collect() if e["name"].startswith("roi_loop_pool") and e["launches"] > 0]
        assert launched == [], launched  # nothing was launched
    finally:
        profile_enable(False)


def test_shapes_outside_the_carrier_forms_are_argument_errors(gpu):
    from wsovod_amd.layers import hip_ops as H

    f, rois, sc = _case(gpu, torch.float32, 256)
    nchw = f.contiguous()  # the reference's layout: the fused entry reads channels-last maps only
    assert not nchw.is_contiguous(memory_format=torch.channels_last)
    for fmt in (torch.float32, H.X2, H.MX):
        with pytest.raises(RuntimeError, match="status 1.*NHWC"):
            H.roi_loop_pool_forward_fused(nchw, rois, SCALE, (7, 7), roi_scale=sc, out_dtype=fmt, need_argmax=False)
    f192 = f[:, :192].contiguous(memory_format=torch.channels_last)
    for fmt in (H.X2, H.MX):
        with pytest.raises(RuntimeError, match="status 1.*multiple of 256"):
            H.roi_loop_pool_forward_fused(f192, rois, SCALE, (7, 7), roi_scale=sc, out_dtype=fmt, need_argmax=False)
    with pytest.raises(RuntimeError, match="status 1.*pw = 7"):
        H.roi_loop_pool_forward_fused(f, rois, SCALE, (7, 5), roi_scale=sc, out_dtype=H.X2, need_argmax=False)
    # the same shapes are fine with a plain output
    out, _ = H.roi_loop_pool_forward_fused(f192, rois, SCALE, (7, 5), roi_scale=sc, out_dtype=torch.float32, need_argmax=False)
    want = H.roi_loop_pool_forward(f192, rois, SCALE, (7, 5))[0] * sc.repeat(3)[:, None, None, None]
    assert same_bits(out.cpu(), want.cpu())
