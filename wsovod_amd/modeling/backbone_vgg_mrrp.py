"""The MRRP form of the VGG16 backbone (the reference's WSOVOD_MRRP_V_16 configs: MODEL.MRRP.MRRP_ON, build_mrrp_vgg_backbone).

Host-side mirror of wsovod/modeling/backbone/vgg_mrrp.py: the last stage, plain5, runs `num_branch` times with ONE set of
weights and one dilation per branch (MRRPPlainBlock, vgg_mrrp.py:128-251: three 3x3 convs with bias and ReLU, no norm, no
shortcut, no pool; conv1 reads the same map for every branch), and its output is `torch.cat` of the branches along N:
(num_branch * N, 512, H, W), branch-major.  The state dict is key for key the plain VGG16's (`plain5.0.conv{j}.{weight,bias}`),
so checkpoints of the two models are interchangeable.  plain1 - plain4, the uint8 entry, the frozen-forward graph and the
"parity_mx" run from plain3 are backbone_vgg.py's.

    hip_conv_branches   one conv of the block over all branches.  "parity" / "parity_mx" own a ONE-launch form of the 256 x 256
                        conv tile (wsovod_gemm_conv_branches / wsovod_gemm_f16mx_conv_branches: tile -> branch in the kernel's
                        prologue, no tile straddles two branches, bit for bit the single-dilation tile's results); it is
                        taken where the measured table BATCHED_UP_TO says it wins, else and in every other precision the
                        branches loop over the single-dilation launches of `hip_conv`.
"""
import os

import torch

from ..config import BACKBONE_REGISTRY
from ..layers import carrier, hip_ops as H, mx_guard
from . import conv as C
from .backbone import CNNBlockBase, forward_precision
from .conv import Conv2d, c2_msra_fill, conv_operand, hip_conv
from .backbone_vgg import VGG16

__all__ = ["MRRPPlainBlock", "MRRPVGG16", "build_mrrp_vgg_backbone", "hip_conv_branches"]

MAX_BRANCHES = 4  # wsovod_conv_branches.dil[4]

# Where the one-launch form is the default: {operand format: largest per-branch image count N at a plain5-sized map up to
# which its median was below the loop's by more than the run-to-run spread} (tools/mrrp_vgg_step.py part (a),
# profiles/mrrp_vgg_step.json; DESIGN.md section 6c-1: at 1 image 0.66 against 1.55 ms and 0.84 against 1.17 ms for the three
# convs, from 4 images on the two forms are within the spread).  0 would be the loop everywhere.
BATCHED_UP_TO = {"f16mx": 1, "bf16x2": 1}


def branch_batched_default(mx, n_images):
    """The form `hip_conv_branches` takes when the caller does not say: WSOVOD_BRANCH_BATCHED = 0 / 1 forces the loop / the one
    launch (A/B runs; read at every call), else the measured table."""
    env = os.environ.get("WSOVOD_BRANCH_BATCHED")
    if env in ("0", "1"):
        return env == "1"
    return n_images <= BATCHED_UP_TO["f16mx" if mx else "bf16x2"]


def _batched_images(conv, Hh, Ww, dilations):
    """Per-branch images the one-launch form takes at once: the n_branch * N operand (input or output, 4 bytes per value)
    plus the largest branch's border in front stays below the buffer-addressing limit (the C side's own check)."""
    pmax = max(dilations)
    per_image = len(dilations) * Hh * Ww * max(conv.in_channels, conv.out_channels) * 4
    return (C.CONV_MAX_OPERAND_BYTES - (pmax * Ww + pmax) * conv.in_channels * 4) // per_image


def hip_conv_branches(x, conv, dilations, shared_input, relu=False, out_fp32=False, batched=None, residual=None,
                      residual_shared=False):
    """`conv` (3x3, stride 1) at every dilation of `dilations` with padding = dilation.  x: with shared_input ONE (N, H, W,
    Cin) NHWC map read by every branch (MRRPPlainBlock.conv1, where x = [x] * num_branch), else (len(dilations) * N, H, W,
    Cin), branch-major.  Returns (len(dilations) * N, H, W, Cout), branch-major: torch.cat([conv(x_b, dilation=d_b)]).
    batched: True / False forces the one-launch form / the loop (None: branch_batched_default).
    residual: a map in x's format added ahead of the ReLU, as `hip_conv`'s -- (len(dilations) * N, H, W, Cout) branch-major,
    or with residual_shared ONE (N, H, W, Cout) map added to every branch (block 0 of an MRRP residual stage, whose
    projection shortcut is the same for every branch: backbone_resnet_mrrp.py).  A 1x1 / stride-1 / unpadded `conv` is taken
    too (the dilations then only count the branches): the Bottleneck's tail conv over the branches with that shared residual."""
    nb = len(dilations)
    if not 1 <= nb <= MAX_BRANCHES:
        raise NotImplementedError(f"wsovod_amd: {nb} MRRP branches (MODEL.MRRP.NUM_BRANCH): at most {MAX_BRANCHES} are built")
    k1 = conv.kernel_size == 1 and conv.padding == 0
    if (conv.kernel_size != 3 and not k1) or conv.stride != 1:
        raise NotImplementedError("wsovod_amd: MRRP branches share a 3x3 / stride-1 conv (or a 1x1 / stride-1 one)")
    NB, Hh, Ww, Cin = x.shape
    N = NB if shared_input else NB // nb
    assert shared_input or NB == nb * N
    assert residual is None or residual.shape == ((N if residual_shared else nb * N), Hh, Ww, conv.out_channels)
    if batched is None:
        batched = H.x2_active() and conv.in_channels % 32 == 0 and conv.out_channels % 32 == 0 \
            and branch_batched_default(H.mx_of(x), N)
    if batched:
        if not H.x2_active() or conv.in_channels % 32 or conv.out_channels % 32:
            raise RuntimeError("hip_conv_branches: the one-launch form exists for bf16x2 / f16mx maps of whole 32-value channel "
                               "groups (\"parity\" / \"parity_mx\")")
        max_n = _batched_images(conv, Hh, Ww, dilations)
        if max_n < 1:
            raise RuntimeError("hip_conv_branches: one image per branch already exceeds the 2 GiB buffer-addressing limit")
        if N > max_n:
            # image blocks per branch, as hip_conv: block i of every branch in one launch, the blocks' branch-major outputs
            # re-interleaved into ONE branch-major map.  Slices and `cat` carry no tag: tagged like their source
            part = lambda t, i, j: carrier.like(t, t[i:j])
            outs = []
            for i in range(0, N, max_n):
                j = min(N, i + max_n)
                xb = part(x, i, j) if shared_input else \
                    carrier.like(x, torch.cat([x[bi * N + i:bi * N + j] for bi in range(nb)]))
                rb = None if residual is None else part(residual, i, j) if residual_shared else \
                    carrier.like(residual, torch.cat([residual[bi * N + i:bi * N + j] for bi in range(nb)]))
                outs.append((j - i, hip_conv_branches(xb, conv, dilations, shared_input, relu=relu, out_fp32=out_fp32, batched=True,
                                                      residual=rb, residual_shared=residual_shared)))
            return carrier.like(outs[0][1], torch.cat([o[bi * n:(bi + 1) * n] for bi in range(nb) for n, o in outs]))
        k = conv.kernel_size
        geom = dict(n_img=N, H=Hh, W=Ww, Cin=Cin, Ho=Hh, Wo=Ww, KH=k, KW=k, stride=1, pad=dilations[0], dil=dilations[0])
        fmt = H.MX if H.mx_of(x) else H.X2
        out_fmt = torch.float32 if out_fp32 else fmt
        w, w_scale, b = conv_operand(conv, fmt, cin_pad=Cin)
        assert residual is None or bool(H.mx_of(residual)) == (fmt == H.MX)
        out = H.conv_branches(x, w, geom, dilations, shared_input=shared_input, b_scale=w_scale, bias=b, relu=relu,
                              out_dtype=out_fmt, residual=None if residual is None else residual.view(-1, conv.out_channels),
                              residual_shared=residual_shared, residual_fmt=fmt)
        if out_fmt == H.MX:
            mx_guard.audit(conv, out)
        return out.view(nb * N, Hh, Ww, conv.out_channels)  # (a whole view of what conv_branches tagged)
    # the loop: one single-dilation conv per branch (its own image blocks above 2 GiB), concatenated along N.  A batch slice is
    # not a whole view and `cat` carries no tag: slices and the output are tagged like their source (layers/carrier.py)
    parts = []
    for bi, d in enumerate(dilations):
        xb = x if shared_input else carrier.like(x, x[bi * N:(bi + 1) * N])
        rb = residual if residual is None or residual_shared else carrier.like(residual, residual[bi * N:(bi + 1) * N])
        parts.append(hip_conv(xb, conv, relu=relu, residual=rb, out_fp32=out_fp32, dilation=None if k1 else int(d)))
    return parts[0] if nb == 1 else carrier.like(parts[0], torch.cat(parts))


class MRRPPlainBlock(CNNBlockBase):
    """vgg_mrrp.py:128-251 with concat_output=True: `num_conv` shared-weight 3x3 convs (bias, no norm) + ReLU per branch."""

    has_pool = False

    def __init__(self, in_channels, out_channels, num_conv=3, stride=1, num_branch=3, dilations=(1, 2, 3), concat_output=True,
                 test_branch_idx=-1, has_pool=False):
        super().__init__(in_channels, out_channels, stride)
        assert 2 <= num_conv < 5 and num_branch == len(dilations)
        if has_pool or not concat_output:
            raise NotImplementedError("wsovod_amd: the MRRP plain block is built as plain5 (no pool, concatenated output)")
        if test_branch_idx != -1:
            raise NotImplementedError(f"wsovod_amd: MODEL.MRRP.TEST_BRANCH_IDX = {test_branch_idx}: every shipped MRRP config "
                                      "runs all branches (-1)")
        self.num_conv, self.num_branch, self.dilations = num_conv, num_branch, tuple(int(d) for d in dilations)
        self.concat_output, self.test_branch_idx, self.pool_stride = concat_output, test_branch_idx, stride
        for j in range(num_conv):  # ordinary parameter holders: the plain VGG16's keys
            conv = Conv2d(in_channels if j == 0 else out_channels, out_channels, 3, stride=1, padding=1, dilation=1, bias=True,
                          norm=None)
            c2_msra_fill(conv)
            setattr(self, f"conv{j + 1}", conv)

    def convs(self):
        return [getattr(self, f"conv{j + 1}") for j in range(self.num_conv)]

    def forward(self, x):
        """x: the block's (N, H, W, Cin) NHWC input -> (num_branch * N, H, W, Cout), branch-major."""
        convs = self.convs()
        for j, conv in enumerate(convs):
            x = hip_conv_branches(x, conv, self.dilations, shared_input=j == 0, relu=True,
                                  out_fp32=j == len(convs) - 1 and getattr(self, "_emits_fp32", False))
        return x


class MRRPVGG16(VGG16):
    """vgg_mrrp.py:254-400: the VGG16 whose plain5 is the MRRP block when "plain5" is in MODEL.MRRP.MRRP_STAGE."""

    def __init__(self, conv5_dilation, freeze_at, num_branch, branch_dilations, mrrp_stage, test_branch_idx, num_classes=None,
                 out_features=None, precision="bf16"):
        branch_dilations = tuple(int(d) for d in branch_dilations)
        if len(branch_dilations) != num_branch:
            raise NotImplementedError(f"wsovod_amd: MODEL.MRRP.BRANCH_DILATIONS = {list(branch_dilations)} does not name "
                                      f"MODEL.MRRP.NUM_BRANCH = {num_branch} dilations")
        if num_branch > MAX_BRANCHES:
            raise NotImplementedError(f"wsovod_amd: MODEL.MRRP.NUM_BRANCH = {num_branch}: at most {MAX_BRANCHES} branches are built")
        if test_branch_idx != -1:
            raise NotImplementedError(f"wsovod_amd: MODEL.MRRP.TEST_BRANCH_IDX = {test_branch_idx}: every shipped MRRP config "
                                      "sets -1 (all branches, in training and in testing)")
        self.num_branch, self.branch_dilations = num_branch, branch_dilations
        self.mrrp_stage, self.test_branch_idx = mrrp_stage, test_branch_idx
        super().__init__(conv5_dilation, freeze_at, num_classes=num_classes, out_features=out_features, precision=precision)

    @property
    def mrrp_stacked(self):
        """The output map is branch-major (plain5 is an MRRP stage): MODEL.MRRP.MRRP_ON must be set for the heads."""
        return "plain5" in self.mrrp_stage

    @property
    def mrrp_num_branch(self):
        """Branches stacked along N in the output map (1: plain5 is not an MRRP stage)."""
        return self.num_branch if "plain5" in self.mrrp_stage else 1

    def _make_block(self, name, kw):
        if name == "plain5" and name in self.mrrp_stage:  # (the reference's `name in self.mrrp_stage` test)
            return MRRPPlainBlock(kw["in_channels"], kw["out_channels"], num_conv=kw["num_conv"], stride=1,
                                  num_branch=self.num_branch, dilations=self.branch_dilations, concat_output=True,
                                  test_branch_idx=self.test_branch_idx, has_pool=False)
        return super()._make_block(name, kw)


@BACKBONE_REGISTRY.register()
def build_mrrp_vgg_backbone(cfg, input_shape):
    """vgg_mrrp.py:403-420."""
    depth = cfg.MODEL.VGG.DEPTH
    if depth != 16:
        raise NotImplementedError(f"wsovod_amd: MODEL.VGG.DEPTH = {depth}: VGG16 is the only depth the reference builds")
    if input_shape.channels != 3:
        raise NotImplementedError("the VGG16 backbone takes 3-channel images")
    m = cfg.MODEL.MRRP
    return MRRPVGG16(cfg.MODEL.VGG.CONV5_DILATION, cfg.MODEL.BACKBONE.FREEZE_AT, m.NUM_BRANCH, m.BRANCH_DILATIONS, m.MRRP_STAGE,
                     m.TEST_BRANCH_IDX, precision=forward_precision(cfg.MODEL.HIP.PRECISION))
