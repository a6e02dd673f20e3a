"""The convolution of the backbones and the RPN head on the HIP implicit-GEMM kernels.

    Conv2d, FrozenBatchNorm2d   parameter holders with detectron2's state-dict layout; `Conv2d.folded` is the weight with the
                                FrozenBN affine folded in, in the kernels' [Cout][kh*kw*Cin] order
    conv_operand                the weight operand of a conv in an operand format (a dtype, bf16x2, f16mx), with or without
                                the block's projection shortcut fused into its rows
    hip_conv                    conv (+ bias + ReLU + residual / fused shortcut + 2x2 pool) on an NHWC map: ONE launch of
                                wsovod_gemm_nt / wsovod_gemm_f16mx; the dilation is an argument, so one set of weights runs
                                at several (backbone_vgg_mrrp.py)
    first_conv                  uint8 canvas -> relu(first conv(normalised image)): the fused first-conv kernels of
                                csrc/stem.hip, or the im2col operand + GEMM
    ResidualBlock               what BasicBlock and BottleneckBlock (backbone.py) share: the tail pool and the ONE forward of
                                a residual block, run by the modules and by the backward's recomputation (conv_backward.py)
"""
import os

import torch
import torch.nn.functional as F
from torch import nn

from ..layers import carrier, hip_ops as H, mx_guard


class FrozenBatchNorm2d(nn.Module):
    """detectron2.layers.FrozenBatchNorm2d: fixed statistics + affine, eps 1e-5 (buffers, not params)."""

    def __init__(self, num_features, eps=1e-5):
        super().__init__()
        self.num_features = num_features
        self.eps = eps
        self.register_buffer("weight", torch.ones(num_features))
        self.register_buffer("bias", torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features) - eps)

    def scale_shift(self):
        scale = self.weight * (self.running_var + self.eps).rsqrt()
        return scale, self.bias - self.running_mean * scale


def get_norm(norm, out_channels):
    if norm is None or (isinstance(norm, str) and len(norm) == 0):
        return None
    if norm == "FrozenBN":
        return FrozenBatchNorm2d(out_channels)
    raise NotImplementedError(f"wsovod_amd backbone supports NORM 'FrozenBN' or '' (got {norm!r})")


def c2_msra_fill(module):
    nn.init.kaiming_normal_(module.weight, mode="fan_out", nonlinearity="relu")
    if module.bias is not None:
        nn.init.constant_(module.bias, 0)


class Conv2d(nn.Module):
    """Parameter holder with detectron2.layers.Conv2d's state-dict layout (weight, bias, norm.*)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, bias=True, norm=None):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding, self.dilation = kernel_size, stride, padding, dilation
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, kernel_size, kernel_size))
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        self.norm = norm
        self._folded = None

    def folded(self, dtype, cin_pad=None):
        """(weight [Cout][kh*kw*Cin] in `dtype` with the FrozenBN scale folded in, fp32 bias)."""
        key = (dtype, cin_pad, self.weight._version, self.weight.device)
        if self._folded is None or self._folded[0] != key:
            with torch.no_grad():
                w = self.weight.float()
                b = self.bias.float() if self.bias is not None else torch.zeros(self.out_channels, device=w.device)
                if self.norm is not None:
                    scale, shift = self.norm.scale_shift()
                    w = w * scale.view(-1, 1, 1, 1)
                    b = b * scale + shift
                w = w.permute(0, 2, 3, 1)  # [Cout][kh][kw][Cin]
                if cin_pad is not None and cin_pad != self.in_channels:
                    w = F.pad(w, (0, cin_pad - self.in_channels))
                wq = w.reshape(self.out_channels, -1).to(dtype).contiguous()
                self._folded = (key, wq, b.contiguous())
        return self._folded[1], self._folded[2]


def _folded_with_shortcut(conv, shortcut, dtype):
    """[W (kh*kw*Cin) | Wshortcut (Cin2)] rows + the summed folded biases: the operand of the conv that contracts the
    block's 1x1 projection shortcut in the same accumulation (wsovod_gemm_desc.A2)."""
    key = (dtype, conv.weight._version, shortcut.weight._version, conv.weight.device)
    c = getattr(conv, "_folded_sc", None)
    if c is None or c[0] != key:
        w, b = conv.folded(dtype)
        ws, bs = shortcut.folded(dtype)
        conv._folded_sc = c = (key, torch.cat([w, ws], dim=1).contiguous(), (b + bs).contiguous())
    return c[1], c[2]


def conv_operand(conv, fmt, cin_pad=None, shortcut=None):
    """The weight operand of `conv` for maps of format `fmt` -- a dtype, H.X2 or H.MX -> (weight, its f16mx row scales or
    None, fp32 bias).  shortcut: the 1x1 projection conv whose rows ride behind the conv's own (_folded_with_shortcut).
    The carriers are encodings of the folded fp32 rows, cached on them (H.x2_cached / H.mx_cached)."""
    dtype = fmt if isinstance(fmt, torch.dtype) else torch.float32
    w, b = conv.folded(dtype, cin_pad=cin_pad) if shortcut is None else _folded_with_shortcut(conv, shortcut, dtype)
    if fmt == H.MX:
        wm, ws = H.mx_cached(w)
        return wm, ws, b
    return (H.x2_cached(w) if fmt == H.X2 else w), None, b


CONV_MAX_OPERAND_BYTES = (1 << 31) - 1  # one buffer resource per NHWC operand (tests lower it to exercise the image blocks)


def hip_conv(x, conv, relu=False, residual=None, pool2=False, shortcut=None, out_fp32=False, dilation=None):
    """x: (N,H,W,Cin) NHWC contiguous in the compute dtype -> (N,Ho,Wo,Cout); with pool2 the MaxPool2d(2, 2) that
    follows the conv in the stem / block tail is applied too -> (N,Ho//2,Wo//2,Cout).  The 64-channel bf16 kernel pools
    in its epilogue (the full-resolution map is never written); every other conv is followed by the pool kernel.
    shortcut = (block input, its 1x1 projection conv): out = conv(x) + projection(input) in one accumulation.
    dilation = d: `conv`'s weights at dilation d with padding d (None: the module's own geometry).

    The operand format follows the mode and the map: a bf16 / fp32 tensor; under "parity" a bf16x2 map (three-MFMA
    products on the bf16x2 weights); under "parity_mx" a unit-scale f16mx map where the run has crossed (fp16 hi*hi +
    block-scaled e4m3 cross terms on the f16mx weights: per-row scales, encoded once -- the stages are frozen or re-encoded
    per optimizer step).  Residual and shortcut input are in the map's format; so is the output, or with out_fp32 under
    "parity" / "parity_mx" real fp32, for the map that leaves the backbone."""
    N, Hh, Ww, Cin = x.shape
    k, s, Cout = conv.kernel_size, conv.stride, conv.out_channels
    p, d = (conv.padding, conv.dilation) if dilation is None else (dilation, dilation)
    Ho = (Hh + 2 * p - d * (k - 1) - 1) // s + 1
    Wo = (Ww + 2 * p - d * (k - 1) - 1) // s + 1
    # the kernels address the NHWC input through one buffer resource (< 2 GiB): larger batches (> 139 images of
    # 800x600 at the 64-channel stem maps) go through in image blocks -- images are independent
    per_image = max(Hh * Ww * Cin, Ho * Wo * Cout) * x.element_size()
    if H.x3_active() in ("full", "fwd") and x.dtype == torch.float32:
        per_image = max(per_image, Hh * Ww * 3 * Cin * 2)  # the operand the kernel addresses is the [hi | hi | lo] bf16 split
    max_n = max(1, CONV_MAX_OPERAND_BYTES // max(per_image, 1))
    if N > max_n:
        # the format of a carrier (layers/carrier.py) is known only through the tensor object's tag, which neither a batch
        # slice (not a whole view) nor `cat` carries: each slice and the concatenated output are tagged like their source
        part = lambda t, i, j: carrier.like(t, t[i:j])
        parts = []
        for i in range(0, N, max_n):
            j = min(N, i + max_n)
            parts.append(hip_conv(part(x, i, j), conv, relu=relu, residual=None if residual is None else part(residual, i, j),
                                  pool2=pool2, shortcut=None if shortcut is None else (part(shortcut[0], i, j), shortcut[1]),
                                  out_fp32=out_fp32, dilation=dilation))
        return carrier.like(parts[0], torch.cat(parts))
    x2 = H.x2_active()
    mx = x2 and H.mx_of(x)
    fmt = H.MX if mx else H.X2 if x2 else x.dtype
    out_fmt = torch.float32 if (x2 and out_fp32) else fmt
    assert not (mx and pool2)
    x_sc = sc = res2d = None
    if shortcut is not None:
        x_sc, sc = shortcut
        assert residual is None and not pool2 and x_sc.shape[:3] == (N, Ho, Wo) and x_sc.shape[3] == sc.in_channels
        assert not mx or H.mx_of(x_sc)
    elif residual is not None:
        assert not mx or H.mx_of(residual)
        res2d = residual.view(N * Ho * Wo, Cout)
    w, w_scale, b = conv_operand(conv, fmt, cin_pad=None if sc is not None else Cin, shortcut=sc)
    geom = dict(n_img=N, H=Hh, W=Ww, Cin=Cin, Ho=Ho, Wo=Wo, KH=k, KW=k, stride=s, pad=p, dil=d)
    # the 64-channel halo kernel pools in its epilogue: the full-resolution map is never written
    fused_pool = (pool2 and not out_fp32 and Cin == 64 and Cout == 64 and (k, s, p, d) == (3, 1, 1, 1)
                  and (x2 or (x.dtype == torch.bfloat16 and (residual is None or residual.dtype == torch.bfloat16))))
    if fused_pool:
        geom["pool"] = 2
    if mx:
        out = H.gemm_mx(x, None, w, w_scale, conv=geom, A2=x_sc, bias=b, relu=relu, residual=res2d,
                        residual_fmt=H.MX if res2d is not None else None, out_dtype=out_fmt)
        if out_fmt == H.MX:
            mx_guard.audit(conv, out)
    else:
        out = H.gemm_nt(x, w, conv=geom, x2=x2, bias=b, relu=relu, residual=res2d, residual_x2=x2, out_dtype=out_fmt, A2=x_sc)
    if fused_pool:
        return out.view(N, Ho // 2, Wo // 2, Cout)
    out = out.view(N, Ho, Wo, Cout)  # (a whole view of what the kernel front tagged)
    return H.maxpool2x2_nhwc(out, 2, x2=out_fmt == H.X2) if pool2 else out


def _fusable_shortcut(sc, x):
    """The block's projection shortcut can ride in its last conv's accumulation: 1x1, stride 1, a whole number of
    K-steps of channels, bf16 / exact-fp32 operands (the bf16x3 modes split their operands and keep the separate launch)."""
    if sc is None or (H.x3_active() and not H.x2_active()) or os.environ.get("WSOVOD_FUSE_SHORTCUT", "1") == "0":
        return False
    kstep = 64 if x.dtype == torch.bfloat16 else 32  # (bf16x2: 32 values = 64 bf16 slots)
    return sc.kernel_size == 1 and sc.stride == 1 and sc.padding == 0 and sc.in_channels % kstep == 0 and x.is_contiguous()


class ResidualBlock:
    """Mixin of BasicBlock and BottleneckBlock (backbone.py): the chain `convs()` = conv1, conv2(, conv3) with ReLUs,
    + `shortcut` (a 1x1 projection conv or None), ReLU, then the optional tail pool that carries the block's stride."""

    def _init_pool(self, has_pool, pool_stride):
        self.has_pool, self.pool_stride = has_pool, pool_stride

    def _pool(self, out):
        if not self.has_pool:
            return out
        # stride 1: ZeroPad2d((0,1,0,1)) + MaxPool2d(2, 1); else MaxPool2d(2, stride)  (resnet_wsl.py:85-92)
        return H.maxpool2x2_nhwc(out, self.pool_stride, zero_pad_br=self.pool_stride == 1, x2=H.x2_active())

    def run(self, x, saving=False):
        """The block on the HIP kernels -> its output; with saving -> (output, [the inputs of conv1, conv2(, conv3)], the
        map ahead of the tail pool): what the backward reads (conv_backward.py).  Both forms launch the same kernels on the
        same bits, but for the stride-2 tail pool behind a 3x3 tail conv (res2 of the BasicBlock nets): the output-only form
        takes it inside hip_conv, where the 64-channel kernel pools in its epilogue and never writes the map the saving
        form keeps (same bits: gemm.hip)."""
        last = getattr(self, "_emits_fp32", False) and not self.has_pool  # "parity": the map that leaves the backbone is real fp32
        *head, tail = self.convs()
        ins, h = [], x
        for conv in head:
            ins.append(h)
            h = hip_conv(h, conv, relu=True)
        ins.append(h)
        pool_in_tail = self.has_pool and self.pool_stride == 2 and tail.kernel_size == 3
        if _fusable_shortcut(self.shortcut, x) and h.shape[:3] == x.shape[:3] and not pool_in_tail:
            # projection shortcut contracted inside the tail conv (K = its own + Cin): no separate 1x1 launch, its output is
            # neither written nor rounded nor re-read as a residual
            out = hip_conv(h, tail, relu=True, shortcut=(x, self.shortcut), out_fp32=last)
        else:
            sc = hip_conv(x, self.shortcut) if self.shortcut is not None else x
            if pool_in_tail and not saving:
                return hip_conv(h, tail, relu=True, residual=sc, pool2=True)
            out = hip_conv(h, tail, relu=True, residual=sc, out_fp32=last)  # out += shortcut; relu
        return (self._pool(out), ins, out) if saving else self._pool(out)


def _im2col_weight(conv, dtype):
    """A 3-channel 3x3 conv's folded [Cout][27] weight in `dtype`, zero-padded to the [Cout][32] operand of the im2col
    order; cached with the fold."""
    wq, b = conv.folded(dtype)
    wpad = getattr(conv, "_w_im2col", None)
    if wpad is None or wpad[0] is not wq:
        w32 = torch.zeros((wq.size(0), 32), dtype=wq.dtype, device=wq.device)
        w32[:, :27] = wq
        conv._w_im2col = wpad = (wq, w32)
    return wpad[1], b


def first_conv(conv, images_u8, sizes, pixel_mean, pixel_std, stride, compute_dtype):
    """uint8 (N,3,Hp,Wp) canvas -> relu(conv(normalised image)), (N,Ho,Wo,Cout) NHWC in the precision's activation format.
    conv: 3x3, pad 1, 3 input channels, stride 1 (VGG16's conv1_1) or 2 (the ResNet stem's conv1).  bf16 and bf16x2 on a
    3 -> 64 conv: ONE kernel from the canvas to the map (bit-identical to im2col + GEMM, no operand pass); else the
    normalised im2col operand (K = 27 padded to 32) + the GEMM."""
    assert conv.in_channels == 3
    x2 = H.x2_active()
    if (x2 or compute_dtype == torch.bfloat16) and conv.out_channels == 64:
        if x2:  # the fused kernel on the bf16x2 encoding of the (64, 32) fp32 weight, bf16x2 output
            w32, b = _im2col_weight(conv, torch.float32)
            kernel = H.stem_conv1_x2 if stride == 2 else H.stem_conv1_s1_x2
            return kernel(images_u8, sizes, pixel_mean, pixel_std, H.x2_cached(w32), b)
        w32, b = _im2col_weight(conv, torch.bfloat16)
        kernel = H.stem_conv1 if stride == 2 else H.stem_conv1_s1
        return kernel(images_u8, sizes, pixel_mean, pixel_std, w32, b)
    a, ho, wo = H.stem_im2col_ex(images_u8, sizes, pixel_mean, pixel_std, compute_dtype, stride)
    w32, b = _im2col_weight(conv, a.dtype)
    return H.gemm_nt(a, w32, bias=b, relu=True, out_dtype=a.dtype).view(images_u8.size(0), ho, wo, conv.out_channels)
