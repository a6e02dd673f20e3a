"""The f16mx implicit-GEMM conv with the request stream's tap state as running offsets (the kernel's TAPTAB form, the
default) against the (r, q, c0) form the launcher keeps behind WSOVOD_MX_TAPTAB=0: the same addresses, so the same bytes.

A 20 x 24 map is 480 pixels = two row tiles, the second one partial; with pad = dilation every border tap is invalid for some
row.  gemm_mx is called directly, so no tile-count threshold stands between these shapes and the f16mx kernel."""
import pytest
import torch

pytestmark = pytest.mark.gpu

HH, WW, CIN, COUT, CIN2 = 20, 24, 128, 256, 64


def _case(gpu, n, dil, shortcut, epi, seed=11):
    """-> run(): the conv's output as raw 32-bit words.  epi: the kernel's epilogue build as the launcher maps it from the
    formats -- 1 = f16mx out, 2 = f16mx out + f16mx residual, 3 = fp32 out + f16mx residual."""
    from wsovod_amd.layers import hip_ops as H

    g = torch.Generator(device=gpu).manual_seed(seed)
    x = torch.relu(torch.randn(n * HH * WW, CIN, device=gpu, generator=g))
    cin2 = CIN2 if shortcut else 0
    w = torch.randn(COUT, 9 * CIN + cin2, device=gpu, generator=g) * 0.03
    bias = torch.randn(COUT, device=gpu, generator=g)
    X = H.mx_encode(x, unit=True)[0].view(n, HH, WW, CIN)
    X2 = H.mx_encode(torch.randn(n * HH * WW, cin2, device=gpu, generator=g), unit=True)[0].view(n, HH, WW, cin2) if cin2 else None
    res = H.mx_encode(torch.randn(n * HH * WW, COUT, device=gpu, generator=g), unit=True)[0] if epi in (2, 3) else None
    W, sw = H.mx_encode(w)
    geom = dict(n_img=n, H=HH, W=WW, Cin=CIN, Ho=HH, Wo=WW, KH=3, KW=3, stride=1, pad=dil, dil=dil)
    fmt = torch.float32 if epi == 3 else H.MX

    def run():
        out = H.gemm_mx(X, None, W, sw, conv=geom, A2=X2, bias=bias, relu=True, residual=res,
                        residual_fmt=H.MX if res is not None else None, out_dtype=fmt)
        torch.cuda.synchronize()
        return out.view(torch.int32).clone()

    return run


def _both(run, monkeypatch):
    monkeypatch.delenv("WSOVOD_MX_TAPTAB", raising=False)
    new = run()
    monkeypatch.setenv("WSOVOD_MX_TAPTAB", "0")
    old = run()
    monkeypatch.delenv("WSOVOD_MX_TAPTAB")
    assert int((new != 0).sum()) > new.numel() // 8  # (a real output, not two empty buffers)
    return new, old


@pytest.mark.parametrize("epi", [1, 2, 3])
@pytest.mark.parametrize("shortcut", [False, True], ids=["plain", "shortcut"])
@pytest.mark.parametrize("dil", [1, 2])
@pytest.mark.parametrize("n", [1, 2])
def test_same_bytes_as_the_tap_state_form(gpu, monkeypatch, n, dil, shortcut, epi):
    """One image (two tiles, the second partial) and two (a tile straddles the image boundary); dilation 1 and 2; with the
    fused projection shortcut's K region behind the taps; each of the three specialised epilogues."""
    new, old = _both(_case(gpu, n, dil, shortcut, epi), monkeypatch)
    assert torch.equal(new, old)


@pytest.mark.parametrize("shortcut", [False, True], ids=["plain", "shortcut"])
@pytest.mark.parametrize("dil", [1, 2])
def test_same_bytes_in_the_split_k_slices(gpu, monkeypatch, dil, shortcut):
    """The last round of tiles as K slices (WSOVOD_MX_TAIL_CUS=3: four tiles on a 'chip' of three CUs -> the fourth tile as
    three slices of 12 / 13 K-steps, which start at taps (1, 0) and (2, 0) / (1, 1) and (2, 2); with the shortcut the last
    slice ends in its region).  fp32 output: the slices' sums leave the kernel unrounded."""
    run = _case(gpu, 2, dil, shortcut, 3)
    monkeypatch.delenv("WSOVOD_MX_TAIL_CUS", raising=False)
    single = run()
    monkeypatch.setenv("WSOVOD_MX_TAIL_CUS", "3")
    new, old = _both(run, monkeypatch)
    assert torch.equal(new, old)
    # the override did send the last tile through the slices: another summation order for its rows, the same sums
    assert torch.equal(new[:768], single[:768]) and not torch.equal(new[768:], single[768:])
    a, b = new.view(torch.float32), single.view(torch.float32)
    assert float((a - b).abs().max()) <= 2e-6 * float(b.abs().max())  # (tests/test_gpu_f16mx.py: split against single launch)


def test_accuracy_against_the_bf16x2_conv(gpu):
    """The same layer on the bf16x2 kernel: within the f16mx format's 2^-14 of the largest |x| * |w| sum, the bound
    tests/test_gpu_f16mx.py holds the f16mx kernels to against exact products (the bf16x2 result is 4 - 8x closer to them)."""
    import torch.nn.functional as F
    from wsovod_amd.layers import hip_ops as H

    torch.manual_seed(5)
    n, dil = 1, 2
    x = torch.relu(torch.randn(n * HH * WW, CIN, device=gpu))
    w = torch.randn(COUT, 9 * CIN, device=gpu) * 0.03
    bias = torch.randn(COUT, device=gpu)
    geom = dict(n_img=n, H=HH, W=WW, Cin=CIN, Ho=HH, Wo=WW, KH=3, KW=3, stride=1, pad=dil, dil=dil)
    W, sw = H.mx_encode(w)
    got = H.gemm_mx(H.mx_encode(x, unit=True)[0].view(n, HH, WW, CIN), None, W, sw, conv=geom, bias=bias, relu=True)
    want = H.gemm_nt(H.x2_encode(x).view(n, HH, WW, CIN), H.x2_encode(w), conv=geom, x2=True, bias=bias, relu=True,
                     out_dtype=torch.float32)
    absprod = F.conv2d(x.view(n, HH, WW, CIN).permute(0, 3, 1, 2).double(),
                       w.abs().view(COUT, 3, 3, CIN).permute(0, 3, 1, 2).double(), None, 1, dil, dil)
    scale = float(absprod.max())
    err = float((got.double() - want.double()).abs().max())
    print(f"f16mx against bf16x2: max |diff| {err:.3e}, bound {2.0 ** -14 * scale:.3e}")
    assert err < 2.0 ** -14 * scale
