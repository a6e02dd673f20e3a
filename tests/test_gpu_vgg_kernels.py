"""-m gpu: the device pieces the VGG16 backbone added -- the stride-1 first conv from the uint8 canvas (csrc/stem.hip:
wsovod_stem_im2col_ex, wsovod_stem_conv1_s1, wsovod_stem_conv1_s1_x2) and the 2x2 max pool on a unit-scale f16mx map
(wsovod_maxpool2x2_nhwc with WSOVOD_F16MX) -- kernel by kernel against torch."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MEAN, STD = [103.939, 116.779, 123.68], [57.375, 57.12, 58.395]


def _ragged(N, Hp, Wp, sizes, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (N, 3, Hp, Wp), dtype=torch.uint8, generator=g)
    return img, torch.tensor(sizes, dtype=torch.int32)


def _normalised(img, sizes, dtype):
    """(x - mean) / std in fp32 (the kernels' table expression), zero outside each image's own size, then `dtype`."""
    x = (img.float() - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)
    for i in range(img.shape[0]):
        x[i, :, int(sizes[i, 0]):, :] = 0
        x[i, :, :, int(sizes[i, 1]):] = 0
    return x.to(dtype)


def _w32(w):
    w32 = torch.zeros(64, 32)
    w32[:, :27] = w.permute(0, 2, 3, 1).reshape(64, 27)  # k = (r*3+q)*3 + c
    return w32


def test_stem_im2col_ex(gpu):
    from wsovod_amd.layers import hip_ops as H

    img, sizes = _ragged(2, 37, 70, [[37, 70], [19, 33]], seed=1)
    a, ho, wo = H.stem_im2col_ex(img.to(gpu), sizes.to(gpu), MEAN, STD, torch.float32, 1)
    assert (ho, wo) == (37, 70) and a.shape == (2 * 37 * 70, 32)
    x = _normalised(img, sizes, torch.float32)
    cols = F.unfold(x, 3, padding=1, stride=1)  # (N, c*9 + r*3 + q, L)
    want = cols.view(2, 3, 9, 37 * 70).permute(0, 3, 2, 1).reshape(2 * 37 * 70, 27)  # k = (r*3+q)*3 + c
    got = a.cpu()
    assert float((got[:, :27] - want).abs().max()) <= 1e-6
    assert float(got[:, 27:].abs().max()) == 0.0
    for dt in (torch.float32, torch.bfloat16):  # stride 2: the bytes of wsovod_stem_im2col
        a2, ho2, wo2 = H.stem_im2col_ex(img.to(gpu), sizes.to(gpu), MEAN, STD, dt, 2)
        b2, ho3, wo3 = H.stem_im2col(img.to(gpu), sizes.to(gpu), MEAN, STD, dt)
        assert (ho2, wo2) == (ho3, wo3) == (19, 35) and torch.equal(a2, b2)


def test_stem_conv1_s1_equals_im2col_plus_gemm(gpu):
    """Partial tiles in both directions (the tile is 8 x 32), more than two tiles across, a second image that ends inside a
    tile, and enough tiles for several workgroups per image; non-zero bias, the ReLU cuts."""
    from wsovod_amd.layers import hip_ops as H

    img, sizes = _ragged(2, 21, 75, [[21, 75], [13, 41]], seed=2)
    g = torch.Generator().manual_seed(3)
    w32 = _w32(torch.randn(64, 3, 3, 3, generator=g) * 0.2).to(torch.bfloat16).to(gpu)
    b = (torch.randn(64, generator=g) * 0.5).to(gpu)
    out = H.stem_conv1_s1(img.to(gpu), sizes.to(gpu), MEAN, STD, w32, b)
    assert out.shape == (2, 21, 75, 64) and out.dtype == torch.bfloat16
    a, _, _ = H.stem_im2col_ex(img.to(gpu), sizes.to(gpu), MEAN, STD, torch.bfloat16, 1)
    want = H.gemm_nt(a, w32, bias=b, relu=True, out_dtype=torch.bfloat16).view(2, 21, 75, 64)
    assert torch.equal(out, want)
    frac0 = float((out == 0).float().mean())
    assert 0.1 < frac0 < 0.9, frac0  # the ReLU cuts, and not everything


def test_stem_conv1_s1_x2_against_fp64(gpu):
    """The tolerance of tests/test_gpu_bf16x2.py::test_stem_conv1_x2_against_fp64 (the stride-2 kernel): 3e-5 of
    max(conv(|x|, |w|))."""
    from wsovod_amd.layers import hip_ops as H

    img, sizes = _ragged(2, 21, 75, [[21, 75], [13, 41]], seed=4)
    g = torch.Generator().manual_seed(5)
    w = torch.randn(64, 3, 3, 3, generator=g) * 0.2
    b = torch.randn(64, generator=g) * 0.5
    x = _normalised(img, sizes, torch.float64)
    pre = F.conv2d(x, w.double(), b.double(), stride=1, padding=1)
    assert float((pre < 0).double().mean()) > 0.1  # negative pre-activations: the ReLU cuts
    ref = torch.relu(pre)
    out = H.stem_conv1_s1_x2(img.to(gpu), sizes.to(gpu), MEAN, STD, H.x2_encode(_w32(w).to(gpu)), b.to(gpu))
    assert out.shape == (2, 21, 75, 64) and H.carrier.fmt_of(out) == H.X2
    got = H.x2_decode(out.view(-1, 64)).view(2, 21, 75, 64).permute(0, 3, 1, 2).cpu().double()
    scale = float(F.conv2d(x.abs(), w.abs().double(), None, stride=1, padding=1).max())
    err = float((got - ref).abs().max())
    print(f"stem_conv1_s1_x2: max |err| {err:.3e}, bound {3e-5 * scale:.3e}")
    assert err < 3e-5 * scale


# ---- the f16mx pool ----
def _coarse_map(N, Hh, Ww, C, seed):
    """fp32 NHWC values on a coarse grid (ties inside most windows) with a fine component on some (so that ql matters)
    and exact zeros."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (N, Hh, Ww, C), generator=g).float() * 0.5
    fine = torch.randint(0, 3, (N, Hh, Ww, C), generator=g).float() * 2.0 ** -13  # below fp16's ulp at 0.5 .. 1.5: lives in ql
    x = x + fine * (torch.rand((N, Hh, Ww, C), generator=g) < 0.5)
    x[torch.rand((N, Hh, Ww, C), generator=g) < 0.15] = 0.0
    return x


def _triples(car):
    """(hi bits int16, q byte, ql byte) per element of an f16mx carrier (..., C), read from its bytes."""
    shape = car.shape
    raw = car.contiguous().view(torch.uint8).view(-1, shape[-1] // 32, 128).cpu()
    hi = raw[:, :, :64].contiguous().view(torch.int16).view(shape)
    return hi, raw[:, :, 64:96].reshape(shape), raw[:, :, 96:].reshape(shape)


@pytest.mark.parametrize("form", ["s2", "s1", "s1_pad"])
@pytest.mark.parametrize("C", [32, 96])
@pytest.mark.parametrize("hw", [(7, 9), (6, 8)])
def test_f16mx_maxpool(gpu, hw, C, form):
    from wsovod_amd.layers import hip_ops as H

    N, (Hh, Ww) = 2, hw
    stride, pad = (2, False) if form == "s2" else (1, form == "s1_pad")
    x = _coarse_map(N, Hh, Ww, C, seed=Hh * 100 + C)
    car, _ = H.mx_encode(x.view(-1, C).to(gpu), unit=True)
    car = H.carrier.tag(car.view(N, Hh, Ww, C), H.MX)
    dec = H.mx_to_f32(car).cpu()  # the values the carrier stands for: hi + ql 2^-11
    assert float((dec - x).abs().max()) < 2.0 ** -14 and float((dec != dec.half().float()).float().mean()) > 0.05
    out = H.maxpool2x2_nhwc(car, stride, zero_pad_br=pad, mx=True)
    assert H.mx_of(out)
    Ho, Wo = ((Hh - 2) // 2 + 1, (Ww - 2) // 2 + 1) if form == "s2" else (Hh, Ww) if pad else (Hh - 1, Ww - 1)
    assert out.shape == (N, Ho, Wo, C)
    src = dec.permute(0, 3, 1, 2)
    if pad:
        src = torch.nn.ZeroPad2d((0, 1, 0, 1))(src)
    want, idx = F.max_pool2d(src, 2, stride, return_indices=True)  # (torch: the first maximum in scan order)
    assert torch.equal(H.mx_to_f32(out).cpu().permute(0, 3, 1, 2), want)
    # the winner's three fields, verbatim: gather the input triples (the padded cells: the all-zero triple) at torch's indices
    ih, iq, il = _triples(car)
    oh, oq, ol = _triples(out)
    Hs, Ws = src.shape[-2:]
    ties = 0
    for name, inp, got in (("hi", ih, oh), ("q", iq, oq), ("ql", il, ol)):
        p = inp.permute(0, 3, 1, 2)
        if pad:
            p = F.pad(p, (0, 1, 0, 1))
        picked = p.reshape(N, C, Hs * Ws).gather(2, idx.reshape(N, C, -1)).view(N, C, Ho, Wo)
        assert torch.equal(got.permute(0, 3, 1, 2), picked), name
    win = F.unfold(src, 2, stride=stride).view(N, C, 4, -1)
    ties = int(((win == win.max(dim=2, keepdim=True).values).sum(2) > 1).sum())
    assert ties > 0  # (the comparison above did decide between equal candidates)
    with pytest.raises(RuntimeError, match="f16mx"):
        H.maxpool2x2_nhwc(torch.zeros(1, 4, 4, 32, device=gpu), 2, mx=True)  # not recorded as an f16mx carrier
