"""GPU: the `_ex` forms of the branch-batched implicit-GEMM conv (wsovod_gemm_conv_branches_ex /
wsovod_gemm_f16mx_conv_branches_ex: residual epilogue, shared or branch-major, and 1x1 filters) against the single-dilation
tile per branch, bit for bit, as tests/test_gpu_vgg_mrrp.py compares the plain forms; the shared work of block 0 against each
branch's own evaluation, bit for bit; and res5 of the MRRP ResNets in both forms against the reference's outputs (g22)."""
import os

import numpy as np
import pytest
import torch

from tests import mrrp_resnet_util as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 3  # rows behind the last branch's M_b that no tile may touch
# (N, H, W): M_b = 35 / 40 (below one tile; at dilation 4 only the centre tap lies inside), 312 (two tiles per branch with a
# masked tail: the next branch starts mid-grid)
MAPS = [(1, 5, 7), (2, 4, 5), (2, 12, 13)]
FILTERS = [(3, 512, 512), (1, 512, 2048)]  # (k, Cin, Cout): res5's 3x3 and the Bottleneck's tail conv
BRANCHES = [(1, 2, 4), (1, 3), (1, 2, 3, 4)]


def _operands(gpu, N, Hh, Ww, k, Cin, Cout, nb, shared_in, shared_res):
    g = torch.Generator().manual_seed(13 * Hh + Ww + Cin + 7 * nb + k)
    x = (torch.relu(torch.randn((N if shared_in else nb * N, Hh, Ww, Cin), generator=g)) * 2.0).to(gpu)
    w = (torch.randn((Cout, k, k, Cin), generator=g) * 0.05).to(gpu)
    bias = torch.randn((Cout,), generator=g).to(gpu)
    res = (torch.randn(((1 if shared_res else nb) * N * Hh * Ww, Cout), generator=g) * 3.0).to(gpu)
    return x, w, bias, res


def _geom(N, Hh, Ww, Cin, k, d):
    return dict(n_img=N, H=Hh, W=Ww, Cin=Cin, Ho=Hh, Wo=Ww, KH=k, KW=k, stride=1, pad=d if k == 3 else 0, dil=d if k == 3 else 1)


def _cases():
    out = []
    for dils in BRANCHES:
        for (N, Hh, Ww) in (MAPS if dils == (1, 2, 4) else MAPS[1:2]):
            for (k, Cin, Cout) in FILTERS:
                for shared_res in (True, False):
                    for relu in (True, False):
                        out.append(pytest.param(N, Hh, Ww, k, Cin, Cout, dils, shared_res, relu,
                                                id=f"{N}x{Hh}x{Ww}-k{k}-{len(dils)}br-{'shared' if shared_res else 'major'}-relu{int(relu)}"))
    return out


def _run(gpu, H, entry, X, W, sw, bias, R, res_fmt, fmts, N, Hh, Ww, k, Cin, Cout, dils, shared_in, shared_res, relu):
    nb, Mb = len(dils), N * Hh * Ww
    for fmt in fmts:
        for with_res in (True, False) if k == 1 else (True,):  # (3x3 without a residual is the plain entry: test_gpu_vgg_mrrp.py)
            buf = torch.full((nb * Mb + GUARD, Cout), -77.25, dtype=torch.float32, device=gpu)
            got = H.conv_branches(X, W, _geom(N, Hh, Ww, Cin, k, dils[0]), dils, shared_input=shared_in, b_scale=sw, bias=bias, relu=relu,
                                  out_dtype=fmt, out=buf, residual=R if with_res else None, residual_shared=shared_res, residual_fmt=res_fmt)
            assert torch.equal(buf[nb * Mb:], torch.full_like(buf[nb * Mb:], -77.25)), "rows past the last branch were written"
            for b, d in enumerate(dils):
                Xb = X if shared_in else X[b * N:(b + 1) * N].contiguous()
                Rb = None if not with_res else R if shared_res else R[b * Mb:(b + 1) * Mb]
                one = entry(Xb, _geom(N, Hh, Ww, Cin, k, d), Rb, fmt)
                assert torch.equal(got[b * Mb:(b + 1) * Mb].view(torch.int32), one.view(torch.int32)), (fmt, with_res, b, d)


@pytest.mark.parametrize("N,Hh,Ww,k,Cin,Cout,dils,shared_res,relu", _cases())
def test_bf16x2_branches_ex(gpu, N, Hh, Ww, k, Cin, Cout, dils, shared_res, relu):
    from wsovod_amd.layers import hip_ops as H

    shared_in = k == 3 and shared_res  # block 0 of the BasicBlock net reads ONE map and adds ONE shortcut
    x, w, bias, res = _operands(gpu, N, Hh, Ww, k, Cin, Cout, len(dils), shared_in, shared_res)
    X = H.x2_encode(x.view(-1, Cin)).view(x.shape)
    W = H.x2_encode(w.reshape(Cout, -1).contiguous())
    R = H.x2_encode(res)

    def one(Xb, geom, Rb, fmt):  # tile_hint: the lean two-phase 256 x 256 tile in its single-launch form (never split along K)
        return H.gemm_nt(Xb, W, conv=geom, x2=True, bias=bias, relu=relu, residual=Rb, residual_x2=True, out_dtype=fmt, tile_hint=2256256)

    _run(gpu, H, one, X, W, None, bias, R, H.X2, (H.X2, torch.float32), N, Hh, Ww, k, Cin, Cout, dils, shared_in, shared_res, relu)
    if k == 3 and relu:  # the fp64 convolution of the decoded operands, the bar of tests/test_gpu_bf16x2.py (3e-5 of the largest output)
        import torch.nn.functional as F

        nb, Mb = len(dils), N * Hh * Ww
        got = H.conv_branches(X, W, _geom(N, Hh, Ww, Cin, k, dils[0]), dils, shared_input=shared_in, bias=bias, relu=True,
                              out_dtype=torch.float32, residual=R, residual_shared=shared_res)
        xd = H.x2_decode(X.view(-1, Cin)).view(x.shape).double()
        wd = H.x2_decode(W).reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2).double()
        rd = H.x2_decode(R).double()
        for b, d in enumerate(dils):
            sl = slice(None) if shared_in else slice(b * N, (b + 1) * N)
            conv = F.conv2d(xd[sl].permute(0, 3, 1, 2), wd, bias.double(), 1, d, d).permute(0, 2, 3, 1).reshape(Mb, Cout)
            want = torch.relu(conv + (rd if shared_res else rd[b * Mb:(b + 1) * Mb]))
            err, scale = float((got[b * Mb:(b + 1) * Mb].double() - want).abs().max()), float(want.abs().max())
            print(f"bf16x2 ex branch {b} dil {d}: err {err:.3e} scale {scale:.3e}")
            assert err < 3e-5 * scale


@pytest.mark.parametrize("N,Hh,Ww,k,Cin,Cout,dils,shared_res,relu", _cases())
def test_f16mx_branches_ex(gpu, monkeypatch, N, Hh, Ww, k, Cin, Cout, dils, shared_res, relu):
    from wsovod_amd.layers import hip_ops as H

    monkeypatch.setenv("WSOVOD_MX_TAIL", "0")  # the single-dilation entry in its single-launch form
    shared_in = k == 3 and shared_res
    x, w, bias, res = _operands(gpu, N, Hh, Ww, k, Cin, Cout, len(dils), shared_in, shared_res)
    X = H.mx_encode(x.view(-1, Cin), unit=True)[0].view(x.shape)
    W, sw = H.mx_encode(w.reshape(Cout, -1).contiguous())
    R = H.mx_encode(res, unit=True)[0]

    def one(Xb, geom, Rb, fmt):
        return H.gemm_mx(Xb, None, W, sw, conv=geom, bias=bias, relu=relu, residual=Rb, residual_fmt=H.MX if Rb is not None else None,
                         out_dtype=fmt)

    _run(gpu, H, one, X, W, sw, bias, R, H.MX, (H.MX, H.X2, torch.float32), N, Hh, Ww, k, Cin, Cout, dils, shared_in, shared_res, relu)


def test_the_ex_entries_refuse_what_they_do_not_build(gpu):
    from wsovod_amd import _lib
    import ctypes as C

    d, br = _lib.GemmDesc(), _lib.ConvBranches()
    d.dtype_in, br.n_branch = _lib.BF16, 3
    assert _lib.lib().wsovod_gemm_conv_branches_ex(C.byref(d), C.byref(br), 0, _lib.stream()) == 3  # WSOVOD_ERR_UNSUPPORTED
    br.n_branch = 5
    assert _lib.lib().wsovod_gemm_conv_branches_ex(C.byref(d), C.byref(br), 0, _lib.stream()) == 1  # WSOVOD_ERR_INVALID_ARGUMENT
    d.dtype_in, br.n_branch = _lib.BF16X2, 3
    d.conv, d.alpha, d.C = 1, 1.0, 16
    d.geom.KH = d.geom.KW = 5
    assert _lib.lib().wsovod_gemm_conv_branches_ex(C.byref(d), C.byref(br), 0, _lib.stream()) == 1  # neither 3x3 nor 1x1


# ---- the blocks and the stage ---------------------------------------------------------------------------------------------
def _net(gpu, depth, precision, dils=U.DILATIONS):
    import wsovod_amd.modeling  # noqa: F401  (registers the builders)
    from wsovod_amd.config import BACKBONE_REGISTRY
    from wsovod_amd.structures import ShapeSpec
    from wsovod_amd.testing import hot_path_cfg

    cfg = hot_path_cfg(depth=depth, mrrp=True, precision=precision, device="cuda:0")
    cfg.MODEL.MRRP.NUM_BRANCH, cfg.MODEL.MRRP.BRANCH_DILATIONS = len(dils), list(dils)
    net = BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg, ShapeSpec(channels=3)).to(gpu).eval()
    net.load_state_dict({k[len("backbone."):]: v for k, v in U.resnet_seeded_state(depth).items()}, strict=True)
    return net


def _res4_carrier(gpu, depth, precision):
    from wsovod_amd.layers import hip_ops as H

    x = U.res4_map(depth).permute(0, 2, 3, 1).contiguous().to(gpu)
    if precision == "fp32":
        return x
    X = H.x2_encode(x.view(-1, x.shape[-1])).view(x.shape)
    return H.mx_from_x2(X) if precision == "parity_mx" else X


def _res5(net, x, precision):
    from wsovod_amd.layers import precision as P

    with torch.no_grad(), P.scope(P.of(precision)):
        return net.res5(x).float().permute(0, 3, 1, 2).cpu().contiguous()


@pytest.fixture(scope="module")
def g22():
    return np.load(os.path.join(ROOT, "tests", "golden", "g22_resnet_mrrp.npz"), allow_pickle=False)


@pytest.mark.parametrize("precision", ["fp32", "parity", "parity_mx"])
@pytest.mark.parametrize("depth", [18, 50])
def test_res5_in_both_forms_against_the_references_output(gpu, monkeypatch, g22, depth, precision):
    """res5 of the MRRP nets on the seeded res4 map of g22, through the loop over `hip_conv` and (parity, parity_mx) through the
    one-launch form, against the REFERENCE's own output with the bar tests/test_gpu_vgg_mrrp.py sets for plain5 (rtol 1e-3 /
    atol 3e-4: both parity precisions are fp32-grade, 2^-16 per product).  The measured errors are printed."""
    want = torch.from_numpy(g22[f"r{depth}_res5"])
    net = _net(gpu, depth, precision)
    x = _res4_carrier(gpu, depth, precision)
    outs = {}
    for form in ("0", "1") if precision != "fp32" else ("0",):
        monkeypatch.setenv("WSOVOD_BRANCH_BATCHED", form)
        outs[form] = _res5(net, x, precision)
        print(f"R{depth} {precision} form {form}: max |err| {float((outs[form] - want).abs().max()):.3e} (max |ref| {float(want.abs().max()):.3f})")
        torch.testing.assert_close(outs[form], want, rtol=1e-3, atol=3e-4)
    if precision == "fp32":  # the one-launch form exists for the parity precisions only: fp32 keeps the loop whatever the override says
        monkeypatch.setenv("WSOVOD_BRANCH_BATCHED", "1")
        assert torch.equal(_res5(net, x, precision), outs["0"])


@pytest.mark.parametrize("form", ["0", "1"])
@pytest.mark.parametrize("precision", ["parity", "parity_mx"])
@pytest.mark.parametrize("depth", [18, 50])
def test_shared_work_of_block_0_equals_each_branchs_own_evaluation(gpu, monkeypatch, depth, precision, form):
    """Block 0 evaluates its projection shortcut (and the Bottleneck's conv1) ONCE for the three branches.  Each branch's own
    evaluation -- the same stage built with that branch's dilation alone, which computes shortcut and conv1 for itself, as the
    reference does per branch -- gives the same bits, for the shortcut / conv1 maps, and for block 0's chunk of that branch."""
    from wsovod_amd.layers import precision as P
    from wsovod_amd.modeling.conv import hip_conv

    monkeypatch.setenv("WSOVOD_BRANCH_BATCHED", form)
    monkeypatch.setenv("WSOVOD_MX_TAIL", "0")
    net = _net(gpu, depth, precision)
    x = _res4_carrier(gpu, depth, precision)
    n = x.shape[0]

    def block0(model):
        with torch.no_grad(), P.scope(P.of(precision)):
            return model.res5[0](x).view(torch.int32).cpu()

    with torch.no_grad(), P.scope(P.of(precision)):
        blk = net.res5[0]
        shared = [(blk.shortcut, False)] + ([(blk.conv1, True)] if depth == 50 else [])
        for conv, relu in shared:  # (what `[self.shortcut(b) for b in x]` computes for x = [x] * num_branch)
            once = hip_conv(x, conv, relu=relu).view(torch.int32).clone()
            for _ in U.DILATIONS:
                assert torch.equal(hip_conv(x, conv, relu=relu).view(torch.int32), once)
    whole = block0(net)
    assert whole.shape[0] == 3 * n
    for b, d in enumerate(U.DILATIONS):
        assert torch.equal(whole[b * n:(b + 1) * n], block0(_net(gpu, depth, precision, dils=(d,)))), (b, d)
