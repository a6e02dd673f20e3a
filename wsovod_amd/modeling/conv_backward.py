"""The backward of a trainable backbone stage (MODEL.BACKBONE.FREEZE_AT = 0 .. 4; reference: resnet_wsl.py:94-110,221-241
under autograd, :530-552) on the HIP kernels themselves.

    tail pool     res2 / res3: the gradient goes to the first maximum of every 2x2 window      wsovod_maxpool2x2_nhwc_backward
    mask          dL/d(pre-activation) = dL/d(out) * [out > 0]              wsovod_mask_transpose
    input grad    a k x k, stride-1, same-size conv IS a conv of the output gradient with the kernel rotated by 180 deg and
                  its channel roles swapped ([Cin][kh'][kw'][Cout]): the implicit-GEMM kernel of the forward pass; 1x1: a GEMM
    weight grad   dW'[co][tap][ci] = sum_p g[p][co] * x[p + tap][ci] = g^T @ im2col(x): the transposed-read contraction
                  (wsovod_gemm_tn) over patch rows (wsovod_im2col_rows); FrozenBN folds w' = w * scale[co], so dw = dW' * scale

Arithmetic: the precision's backward grade -- plain bf16 MFMA products with fp32 accumulation for "bf16" / "parity" (on
the hi halves of bf16x2 maps), exact-fp32 MFMA for "fp32".  The stage's activations are RE-COMPUTED by the forward's own code
(`ResidualBlock.run`, conv.py: bit-identical to the forward that produced the loss, so the ReLU masks and pool winners are
the forward's own).  The "bf16x3" modes, which keep their operands in fp32 tensors and split on the fly, and
WSOVOD_HIP_CONV_BACKWARD = 0 take the earlier form instead: the stage re-evaluated from its saved input with torch's GPU
convolution in fp32 under autograd (`_torch_block`) -- there a mask or pool winner can differ from the forward's where two
candidates lie within the forward's rounding.
"""
import os

import torch
import torch.nn.functional as F

from ..layers import carrier, hip_ops as H, precision as P
from .conv import ResidualBlock, hip_conv


def _torch_conv(conv, x):
    """conv + FrozenBN as torch ops on NCHW fp32 (resnet_wsl.py / detectron2 Conv2d.forward): the backward's restatement."""
    y = F.conv2d(x, conv.weight, conv.bias, conv.stride, conv.padding, conv.dilation)
    if conv.norm is not None:
        scale, shift = conv.norm.scale_shift()
        y = y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    return y


def _torch_block(block, x):
    """resnet_wsl.py:94-110 (BasicBlock) / :224-241 (BottleneckBlock) in torch ops."""
    *head, tail = block.convs()
    out = x
    for conv in head:
        out = F.relu(_torch_conv(conv, out))
    out = _torch_conv(tail, out)
    out = F.relu(out + (_torch_conv(block.shortcut, x) if block.shortcut is not None else x))
    if block.has_pool:  # resnet_wsl.py:85-92
        out = F.max_pool2d(F.pad(out, (0, 1, 0, 1)), 2, 1) if block.pool_stride == 1 else F.max_pool2d(out, 2, block.pool_stride)
    return out


def _hip_backward_ok(stage, x3):
    if os.environ.get("WSOVOD_HIP_CONV_BACKWARD", "1") == "0" or x3 in ("full", "fwd"):
        return False  # (the bf16x3 modes keep their operands in fp32 tensors and split on the fly: torch re-evaluation)
    for b in stage.children():
        if not isinstance(b, ResidualBlock):
            return False
        for c in (*b.convs(), b.shortcut):
            if c is not None and (c.stride != 1 or c.bias is not None or 2 * c.padding != c.dilation * (c.kernel_size - 1)
                                  or c.in_channels % 64 or c.out_channels % 64):
                return False
    return True


WGRAD_PATCH_BYTES = 1 << 30  # (tests lower it to exercise the row blocks)


def _masked(dy, y, cd):
    """dL/d(pre-activation) of y = relu(.): (P, C) in the compute dtype `cd` (dy fp32, y the forward's own output map)."""
    C = dy.shape[-1]
    P = dy.numel() // C
    if y.dtype == torch.bfloat16 and dy.dtype != torch.bfloat16:
        dy = dy.to(torch.bfloat16)  # (the mask kernel takes dy in y's dtype; "bf16" precision: bf16 gradients anyway)
    return H.mask_transpose(dy.reshape(P, C), y.reshape(P, C), 1.0, cd, want_plain=True, want_t=False,
                            y_x2=carrier.fmt_of(y) == H.X2)[0]


def _conv_dgrad(g2d, conv, N, Hh, Ww, cd):
    """g2d: (N*H*W, Cout) in cd -> dL/d(input) (N*H*W, Cin) fp32."""
    k, d = conv.kernel_size, conv.dilation
    w, _ = conv.folded(torch.float32)  # [Cout][kh*kw*Cin]
    Co, Ci = conv.out_channels, conv.in_channels
    if k == 1:
        return H.gemm_nt(g2d, w.t().contiguous().to(cd), out_dtype=torch.float32)
    wt = w.view(Co, k, k, Ci).flip(1, 2).permute(3, 1, 2, 0).reshape(Ci, k * k * Co).contiguous().to(cd)
    geom = dict(n_img=N, H=Hh, W=Ww, Cin=Co, Ho=Hh, Wo=Ww, KH=k, KW=k, stride=1, pad=conv.padding, dil=d)
    return H.gemm_nt(g2d.view(N, Hh, Ww, Co), wt, conv=geom, out_dtype=torch.float32)


def _conv_wgrad(g2d, xin, conv, cd):
    """g2d (P, Cout) in cd; xin: the conv's NHWC input as the forward left it (bf16 / fp32 / bf16x2 carrier) -> dL/dw in
    the parameter's own layout (Cout, Cin, kh, kw), FrozenBN scale applied."""
    k = conv.kernel_size
    N, Hh, Ww, Ci = xin.shape
    P = N * Hh * Ww
    x2 = carrier.fmt_of(xin) == H.X2  # (a bf16x2 carrier and a real fp32 map have the same dtype and shape: the tag tells)
    # patch rows are materialised in blocks of at most ~1 GiB (the stem's 64-channel convs at 32 images would be 8.8 GB at
    # once): the blocks' contributions accumulate into dW
    step = P if k == 1 else max(64, (WGRAD_PATCH_BYTES // (k * k * Ci * xin.element_size())) // 64 * 64)
    dw = torch.empty((conv.out_channels, k * k * Ci), dtype=torch.float32, device=xin.device)
    for a in range(0, P, step):
        b = min(P, a + step)
        if k == 1:
            patches = xin.reshape(P, Ci)
        else:
            rows = torch.arange(a, b, dtype=torch.int64, device=xin.device)
            patches = H.im2col_rows(xin, rows, k, 1, conv.padding, conv.dilation)  # (b - a, k*k*Ci), tap-major then channel
        gb = g2d[a:b]
        if cd == torch.float32:
            Pp = (b - a + 63) // 64 * 64
            H.gemm_nt(H.transpose_cast(gb, torch.float32, ld_dst=Pp), H.transpose_cast(patches, torch.float32, ld_dst=Pp),
                      out=dw, accumulate=a > 0)
        else:
            H.gemm_tn(gb, patches, out=dw, accumulate=a > 0, q_x2=x2)  # of a bf16x2 map the hi halves are read
        del patches
    dw = dw.view(conv.out_channels, k, k, Ci).permute(0, 3, 1, 2)
    if conv.norm is not None:
        dw = dw * conv.norm.scale_shift()[0].view(-1, 1, 1, 1)
    return dw.contiguous()


def _block_forward_saving(block, x):
    """The block's forward keeping what the backward reads -> (out, [inputs of conv1, conv2(, conv3)], the map the tail
    pool reads -- `out` itself without one): the saving form of the block's one forward."""
    return block.run(x, saving=True)


def _block_backward(block, ins, out, dy, cd, need_dx):
    """dy: dL/d(out) (N,H,W,C) fp32 -> (dL/d(block input) (N,H,W,Cin) fp32 or None, {conv module: dL/dw})."""
    N, Hh, Ww, _ = out.shape
    convs = block.convs()
    grads = {}
    if block.has_pool:  # `out` is the map the tail pool read: route dy back through the pool first
        dy = H.maxpool2x2_nhwc_backward(out, dy.contiguous(), block.pool_stride, zero_pad_br=block.pool_stride == 1,
                                        x2=carrier.fmt_of(out) == H.X2)
    g = _masked(dy.contiguous(), out, cd)  # through the block's last ReLU: gradient of conv_tail(h) + shortcut(x)
    g_tail = g
    for i in range(len(convs) - 1, -1, -1):
        conv, xin = convs[i], ins[i]
        if conv.weight.requires_grad:
            grads[conv] = _conv_wgrad(g, xin, conv, cd)
        if i == 0 and not need_dx:
            dx = None
            break
        dx = _conv_dgrad(g, conv, N, Hh, Ww, cd)  # fp32 (P, Cin of this conv)
        if i > 0:
            g = _masked(dx.view(N, Hh, Ww, -1), xin, cd)  # through the ReLU that produced this conv's input
    sc = block.shortcut
    if sc is not None:
        if sc.weight.requires_grad:
            grads[sc] = _conv_wgrad(g_tail, ins[0], sc, cd)
        if need_dx:
            dx = dx + _conv_dgrad(g_tail, sc, N, Hh, Ww, cd)
    elif need_dx:
        dx = dx + (g_tail.float() if g_tail.dtype != torch.float32 else g_tail)
    return (dx.view(N, Hh, Ww, -1) if dx is not None else None), grads


class _TrainableStage(torch.autograd.Function):
    """One backbone stage with trainable weights.  forward: the HIP kernels (as for a frozen stage).  backward: on the
    HIP kernels too (`_backward_hip`: recomputed activations, then block by block from the last), or -- the bf16x3 modes,
    `_hip_backward_ok` -- the stage re-evaluated from its saved input in fp32 torch ops on the GPU under autograd.  That
    re-evaluation is fp32 while the forward that produced the loss ran in the model's precision: a ReLU mask or max-pool
    winner can differ from the forward's where two candidates lie within the forward's rounding, so its gradient is that
    of a slightly different function (tests/test_gpu_freeze_at.py)."""

    @staticmethod
    def forward(ctx, stage, x3, x, *params):
        with torch.no_grad(), H.x3_mode(x3):
            y = stage(x)
        ctx.stage, ctx.x3 = stage, x3
        ctx.save_for_backward(x, *params)
        return y

    @staticmethod
    def _backward_hip(ctx, dy, x, params):
        stage = ctx.stage
        cd = torch.float32 if (ctx.x3 is False and x.dtype == torch.float32) else torch.bfloat16
        blocks = list(stage.children())
        with torch.no_grad():
            with H.x3_mode(ctx.x3):  # the forward's own kernels again: bit-identical activations, hence the forward's own masks
                # x came through ctx.saved_tensors, which does not promise to hand back the tagged object: its format is stated
                # again from the mode.  Every other map of the stage is a fresh kernel output, tagged by its front; the real-fp32
                # map that leaves the backbone is untagged by construction
                acts, cur = [], (carrier.tag(x, H.X2) if H.x2_active() else x)
                for b in blocks:
                    nxt, ins, out = _block_forward_saving(b, cur)
                    acts.append((ins, out))
                    cur = nxt
            grads = {}
            g = dy.float() if dy.dtype != torch.float32 else dy
            with H.x3_mode(False):
                for bi in range(len(blocks) - 1, -1, -1):
                    ins, out = acts[bi]
                    need_dx = bi > 0 or ctx.needs_input_grad[2]
                    g, gb = _block_backward(blocks[bi], ins, out, g, cd, need_dx)
                    grads.update({id(c.weight): v for c, v in gb.items()})
        dx = None
        if ctx.needs_input_grad[2] and g is not None:
            dx = g if x.dtype == torch.float32 else g.to(x.dtype)
        return (None, None, dx, *[grads.get(id(p)) if p.requires_grad else None for p in params])

    @staticmethod
    def backward(ctx, dy):
        x, *params = ctx.saved_tensors
        if _hip_backward_ok(ctx.stage, ctx.x3):
            return _TrainableStage._backward_hip(ctx, dy, x, params)
        with torch.no_grad():  # the saved map in its on-device format (bf16x2 carrier / bf16 / fp32 NHWC) -> fp32 NCHW
            x32 = H.x2_decode(x.reshape(-1, x.shape[-1])).view(x.shape) if P.is_x2(ctx.x3) else x.float()
            x32 = x32.permute(0, 3, 1, 2).contiguous()
        need_dx = ctx.needs_input_grad[2]
        x32.requires_grad_(need_dx)
        with torch.enable_grad():
            y = x32
            for block in ctx.stage.children():
                y = _torch_block(block, y)
        wanted = ([x32] if need_dx else []) + [p for p in params if p.requires_grad]
        grads = list(torch.autograd.grad(y, wanted, dy.float().permute(0, 3, 1, 2), allow_unused=True))
        dx = grads.pop(0).permute(0, 2, 3, 1).contiguous().to(torch.float32 if P.is_x2(ctx.x3) else x.dtype) if need_dx else None
        it = iter(grads)
        return (None, None, dx, *[next(it) if p.requires_grad else None for p in params])


class _TrainableStem(torch.autograd.Function):
    """MODEL.BACKBONE.FREEZE_AT = 0: the stem with trainable weights.  forward: the fused uint8 -> conv1 kernel and
    the 64-channel convs as for a frozen stem.  backward: the stem's activations recomputed by the same kernels, then pool
    backward -> mask -> weight / input gradients of conv3 and conv2 as in the residual stages -> conv1's weight gradient as
    g^T @ (normalised im2col rows of the image, wsovod_stem_im2col); the image itself takes no gradient."""

    @staticmethod
    def forward(ctx, net, x3, images_u8, sizes, mean, std, *params):
        with torch.no_grad(), H.x3_mode(x3):
            out = net._stem_uint8(images_u8, sizes, mean, std)
        ctx.net, ctx.x3, ctx.norm = net, x3, (mean, std)
        ctx.save_for_backward(images_u8, sizes, *params)
        return out

    @staticmethod
    def backward(ctx, dy):
        images_u8, sizes, *params = ctx.saved_tensors
        net, stem = ctx.net, ctx.net.stem
        mean, std = ctx.norm
        cd = torch.float32 if (ctx.x3 is False and net.compute_dtype == torch.float32) else torch.bfloat16
        with torch.no_grad():
            with H.x3_mode(ctx.x3):
                x2 = H.x2_active()
                a1 = net._stem_conv1(images_u8, sizes, mean, std)  # (bf16x2 maps are tagged by the kernel fronts)
                a2 = hip_conv(a1, stem.conv2, relu=True)
                a3 = hip_conv(a2, stem.conv3, relu=True)  # (the forward pools in this conv's epilogue: same bits)
            grads = {}
            with H.x3_mode(False):
                N, Hh, Ww, _ = a3.shape
                g = H.maxpool2x2_nhwc_backward(a3, (dy.float() if dy.dtype != torch.float32 else dy).contiguous(), 2, x2=x2)
                g = _masked(g, a3, cd)
                for conv, xin, yin in ((stem.conv3, a2, a2), (stem.conv2, a1, a1)):
                    if conv.weight.requires_grad:
                        grads[id(conv.weight)] = _conv_wgrad(g, xin, conv, cd)
                    g = _masked(_conv_dgrad(g, conv, N, Hh, Ww, cd).view(N, Hh, Ww, -1), yin, cd)
                if stem.conv1.weight.requires_grad:
                    patches, _, _ = H.stem_im2col(images_u8, sizes, mean, std, cd)  # (P, 32): [kh][kw][cin] + 5 zero columns
                    if cd == torch.float32:
                        Pp = (patches.size(0) + 63) // 64 * 64
                        dw = H.gemm_nt(H.transpose_cast(g, torch.float32, ld_dst=Pp),
                                       H.transpose_cast(patches, torch.float32, ld_dst=Pp), out_dtype=torch.float32)
                    else:
                        dw = H.gemm_tn(g, patches)
                    dw = dw[:, :27].reshape(stem.conv1.out_channels, 3, 3, 3).permute(0, 3, 1, 2)
                    if stem.conv1.norm is not None:
                        dw = dw * stem.conv1.norm.scale_shift()[0].view(-1, 1, 1, 1)
                    grads[id(stem.conv1.weight)] = dw.contiguous()
        return (None, None, None, None, None, None, *[grads.get(id(p)) if p.requires_grad else None for p in params])
