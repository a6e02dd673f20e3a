"""GPU: the branch-batched implicit-GEMM conv (wsovod_gemm_conv_branches / wsovod_gemm_f16mx_conv_branches) and the MRRP
VGG16 backbone built on it (modeling/backbone_vgg_mrrp.py).  Tolerances are those of the single-dilation conv cases of
tests/test_gpu_f16mx.py (1e-5 of the largest output against the fp64 three-plane convolution) and tests/test_gpu_bf16x2.py
(3e-5 of the largest output against the fp64 convolution), and of tests/test_gpu_vgg_model.py for plain5 in fp32."""
import pytest
import torch
import torch.nn.functional as F

from tests import mrrp_util, vgg_util

pytestmark = pytest.mark.gpu

GUARD = 3  # rows behind the last branch's M_b that no tile may touch
# (N, H, W): M_b = 20 / 40 (far below one tile), 143 (one partial tile per branch), 874 (three full tiles plus a tail: a
# branch boundary falls inside what would be one tile of the flat batch)
MAPS = [(1, 4, 5), (2, 4, 5), (1, 13, 11), (2, 19, 23)]
CHANNELS = [(512, 512), (64, 288)]
DILATIONS = [(1, 2, 4), (1, 2, 3), (2,), (1, 1, 1, 1)]


def _operands(gpu, N, Hh, Ww, Cin, Cout, nb, shared):
    g = torch.Generator().manual_seed(11 * Hh + Ww + Cin + nb)
    x = (torch.relu(torch.randn((N if shared else nb * N, Hh, Ww, Cin), generator=g)) * 2.0).to(gpu)
    w = (torch.randn((Cout, 3, 3, Cin), generator=g) * 0.05).to(gpu)
    bias = torch.randn((Cout,), generator=g).to(gpu)
    return x, w, bias


def _geom(N, Hh, Ww, Cin, d):
    return dict(n_img=N, H=Hh, W=Ww, Cin=Cin, Ho=Hh, Wo=Ww, KH=3, KW=3, stride=1, pad=d, dil=d)


def _padded(gpu, rows, Cout):
    return torch.full((rows + GUARD, Cout), -77.25, dtype=torch.float32, device=gpu)


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("dils", DILATIONS)
@pytest.mark.parametrize("Cin,Cout", CHANNELS)
@pytest.mark.parametrize("N,Hh,Ww", MAPS)
def test_f16mx_branches(gpu, monkeypatch, N, Hh, Ww, Cin, Cout, dils, shared):
    from wsovod_amd.layers import hip_ops as H

    monkeypatch.setenv("WSOVOD_MX_TAIL", "0")  # the single-dilation entry in its single-launch form
    nb, Mb = len(dils), N * Hh * Ww
    x, w, bias = _operands(gpu, N, Hh, Ww, Cin, Cout, nb, shared)
    X = H.mx_encode(x.view(-1, Cin), unit=True)[0].view(x.shape)
    W, sw = H.mx_encode(w.reshape(Cout, -1).contiguous())
    hx, qx, lx = (t.view(x.shape) for t in H.mx_decode(X.view(-1, Cin)))
    hw, qw, lw = (t.reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2).double() for t in H.mx_decode(W, sw))
    for fmt in (H.MX, H.X2, torch.float32):
        buf = _padded(gpu, nb * Mb, Cout)
        got = H.conv_branches(X, W, _geom(N, Hh, Ww, Cin, dils[0]), dils, shared_input=shared, b_scale=sw, bias=bias, relu=True,
                              out_dtype=fmt, out=buf)
        assert torch.equal(buf[nb * Mb:], torch.full_like(buf[nb * Mb:], -77.25)), "rows past the last branch were written"
        for b, d in enumerate(dils):
            Xb = X if shared else X[b * N:(b + 1) * N].contiguous()
            one = H.gemm_mx(Xb, None, W, sw, conv=_geom(N, Hh, Ww, Cin, d), bias=bias, relu=True, out_dtype=fmt)
            assert torch.equal(got[b * Mb:(b + 1) * Mb].view(torch.int32), one.view(torch.int32)), (fmt, b, d)
        if fmt is torch.float32:
            for b, d in enumerate(dils):
                sl = slice(None) if shared else slice(b * N, (b + 1) * N)
                conv = lambda xp, wp: F.conv2d(xp[sl].double().permute(0, 3, 1, 2), wp, None, 1, d, d).permute(0, 2, 3, 1)
                want = torch.relu(conv(hx, hw) + conv(qx, lw) + conv(lx, qw) + bias.double()).reshape(Mb, Cout)
                err, scale = float((got[b * Mb:(b + 1) * Mb].double() - want).abs().max()), float(want.abs().max())
                print(f"f16mx branch {b} dil {d}: err {err:.3e} scale {scale:.3e}")
                assert err < 1e-5 * scale


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("dils", DILATIONS)
@pytest.mark.parametrize("Cin,Cout", CHANNELS)
@pytest.mark.parametrize("N,Hh,Ww", MAPS)
def test_bf16x2_branches(gpu, N, Hh, Ww, Cin, Cout, dils, shared):
    from wsovod_amd.layers import hip_ops as H

    nb, Mb = len(dils), N * Hh * Ww
    x, w, bias = _operands(gpu, N, Hh, Ww, Cin, Cout, nb, shared)
    X = H.x2_encode(x.view(-1, Cin)).view(x.shape)
    W = H.x2_encode(w.reshape(Cout, -1).contiguous())
    xd = H.x2_decode(X.view(-1, Cin)).view(x.shape).double()
    wd = H.x2_decode(W).reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2).double()
    for fmt in (H.X2, torch.float32):
        buf = _padded(gpu, nb * Mb, Cout)
        got = H.conv_branches(X, W, _geom(N, Hh, Ww, Cin, dils[0]), dils, shared_input=shared, bias=bias, relu=True,
                              out_dtype=fmt, out=buf)
        assert torch.equal(buf[nb * Mb:], torch.full_like(buf[nb * Mb:], -77.25)), "rows past the last branch were written"
        for b, d in enumerate(dils):
            Xb = X if shared else X[b * N:(b + 1) * N].contiguous()
            # tile_hint: the lean two-phase 256 x 256 tile in its single-launch form (a named tile is never split along K)
            one = H.gemm_nt(Xb, W, conv=_geom(N, Hh, Ww, Cin, d), x2=True, bias=bias, relu=True, out_dtype=fmt, tile_hint=2256256)
            assert torch.equal(got[b * Mb:(b + 1) * Mb].view(torch.int32), one.view(torch.int32)), (fmt, b, d)
        if fmt is torch.float32:
            for b, d in enumerate(dils):
                sl = slice(None) if shared else slice(b * N, (b + 1) * N)
                want = torch.relu(F.conv2d(xd[sl].permute(0, 3, 1, 2), wd, bias.double(), 1, d, d)).permute(0, 2, 3, 1).reshape(Mb, Cout)
                err, scale = float((got[b * Mb:(b + 1) * Mb].double() - want).abs().max()), float(want.abs().max())
                print(f"bf16x2 branch {b} dil {d}: err {err:.3e} scale {scale:.3e}")
                assert err < 3e-5 * scale


def test_other_operand_types_are_refused_by_the_one_launch_entry(gpu):
    from wsovod_amd.layers import hip_ops as H
    from wsovod_amd import _lib
    import ctypes as C

    d, br = _lib.GemmDesc(), _lib.ConvBranches()
    d.dtype_in, br.n_branch = _lib.BF16, 3
    assert _lib.lib().wsovod_gemm_conv_branches(C.byref(d), C.byref(br), _lib.stream()) == 3  # WSOVOD_ERR_UNSUPPORTED
    br.n_branch = 5
    assert _lib.lib().wsovod_gemm_conv_branches(C.byref(d), C.byref(br), _lib.stream()) == 1  # WSOVOD_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def mrrp_refs():
    """The reference's own outputs (g21: tests/golden/make_golden_mrrp_vgg.py) for both dilation sets on both inputs; the
    restatement is tied to them on the CPU side (tests/test_vgg_mrrp_host.py) and used below for the branch-order check."""
    import os
    import numpy as np

    g21 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_vgg16_mrrp.npz"), allow_pickle=False)
    sd = vgg_util.vgg_seeded_state()
    return sd, [(x, {dl: torch.from_numpy(g21["d%s_plain5_%d" % ("".join(map(str, dl)), i)]) for dl in ((1, 2, 4), (1, 2, 3))})
                for i, x in enumerate(vgg_util.vgg_inputs())]


def _model(gpu, precision, dils, sd):
    from wsovod_amd.modeling.backbone_vgg_mrrp import MRRPVGG16

    net = MRRPVGG16(2, 5, len(dils), dils, "plain5", -1, precision=precision).to(gpu).eval()
    net.load_state_dict(sd, strict=True)
    return net


@pytest.mark.parametrize("dils", [(1, 2, 4), (1, 2, 3)])
def test_backbone_fp32_equals_the_restatement_branch_by_branch(gpu, mrrp_refs, dils):
    sd, refs = mrrp_refs
    net = _model(gpu, "fp32", dils, sd)
    for x, want in refs:
        got = net(x.to(gpu))["plain5"].float().cpu()
        assert tuple(got.shape) == tuple(want[dils].shape) and got.shape[0] == 3
        torch.testing.assert_close(got, want[dils], rtol=1e-3, atol=3e-4)  # the reference's own output (g21)
        for b, d in enumerate(dils):  # branch order: chunk b is the PLAIN model's restatement with plain5 dilation d_b
            torch.testing.assert_close(got[b:b + 1], mrrp_util.vgg16_mrrp_ref(sd, x, dilations=(d,)), rtol=1e-3, atol=3e-4)
        torch.testing.assert_close(got[1:2], vgg_util.vgg16_ref(sd, x, conv5_dilation=2), rtol=1e-3, atol=3e-4)


@pytest.mark.parametrize("precision", ["parity", "parity_mx"])
def test_backbone_parity_precisions_in_both_forms(gpu, monkeypatch, mrrp_refs, precision):
    """plain5 of the parity precisions through the one-launch form and through the loop over `hip_conv`, against the fp32
    reference's outputs (g21) with the bar tests/test_gpu_vgg_model.py sets for the backbone map (rtol 1e-3 / atol 3e-4: both precisions
    are fp32-grade, 2^-16 per product).  At these sizes the loop takes other tiles than the one-launch form (and may split
    K), so the two forms are held to the same bar against each other, not to equal bits: the kernel tests above pin the bits."""
    from wsovod_amd.modeling import backbone_vgg_mrrp as M
    from wsovod_amd.modeling.backbone import FrozenForwardMixin

    monkeypatch.setattr(FrozenForwardMixin, "MX_MIN_TILES", 1)
    sd, refs = mrrp_refs
    net = _model(gpu, precision, (1, 2, 4), sd)
    for x, want in refs:
        outs = {}
        for form in ("0", "1"):
            monkeypatch.setenv("WSOVOD_BRANCH_BATCHED", form)
            outs[form] = net(x.to(gpu))["plain5"].float().cpu().contiguous()
            print(f"{precision} form {form}: max err {float((outs[form] - want[(1, 2, 4)]).abs().max()):.3e}")
            torch.testing.assert_close(outs[form], want[(1, 2, 4)], rtol=1e-3, atol=3e-4)
        torch.testing.assert_close(outs["1"], outs["0"], rtol=1e-3, atol=3e-4)
