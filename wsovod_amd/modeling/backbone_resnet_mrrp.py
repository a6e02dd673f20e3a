"""The MRRP form of the WSL ResNet backbone (the reference's WSOVOD_MRRP_WSR_18/50_DC5 configs: MODEL.MRRP.MRRP_ON,
build_mrrp_wsl_resnet_backbone).

Host-side mirror of wsovod/modeling/backbone/resnet_wsl_mrrp.py: the blocks of the last stage, res5, run `num_branch` times
with ONE set of weights and one dilation per branch (MRRPBasicBlock :122-239: both 3x3 convs branched; MRRPBottleneckBlock
:373-522: conv1 and conv3 ordinary 1x1 convs, only conv2 branched; stride 1, no pool), and the stage's output is `torch.cat`
of the branches along N: (num_branch * N, C, H, W), branch-major, stride 8.  The weights live in the plain blocks' holders: the
state dict is key for key `build_wsl_resnet_backbone`'s (the reference's MRRPConv also names its tensors `weight` and
`norm.*`), so checkpoints of the two models are interchangeable.  The stem, res2 - res4, the uint8 entry, the frozen-forward
graph and the "parity_mx" run with its gates are backbone.py's.

Shared work is done once.  Block 0 of the stage reads the SAME map in every branch; the reference nevertheless evaluates its
projection shortcut once per branch, and in the Bottleneck conv1 too.  Here each runs once: the values are identical across
branches, so the result is bit for bit what the per-branch evaluation gives, and the one shortcut map is a residual SHARED by
the branches (`hip_conv_branches(..., residual_shared=True)`).  From block 1 on, inputs and residuals are branch-major, and
the Bottleneck's 1x1 convs are ordinary convs over the num_branch * N maps.
"""
import os

from ..config import BACKBONE_REGISTRY
from ..layers import hip_ops as H
from .backbone import BasicBlock, BottleneckBlock, ResNet, forward_precision, wsl_resnet_stem_and_stages
from .backbone_vgg_mrrp import MAX_BRANCHES, hip_conv_branches
from .conv import hip_conv

__all__ = ["MRRPBasicBlock", "MRRPBottleneckBlock", "MRRPResNet", "build_mrrp_wsl_resnet_backbone"]

# Where the one-launch form of a block's branched convs is the default: {block kind: {operand format: largest per-branch
# image count N at the res5 map of an 800 x 600 image up to which its median was below the loop's by more than the run-to-run
# spread}} (tools/mrrp_resnet_step.py part (a), profiles/mrrp_resnet_step.json; DESIGN.md section 6c-2: f16mx ahead at every
# measured size, 1 - 32 images, on both nets; bf16x2 ahead at 1 image on the BasicBlock stage and at 1 - 8 images on the
# Bottleneck stage, within the spread beyond).  0 would be the loop everywhere; 32 is the largest size measured.
BATCHED_UP_TO = {"basic": {"f16mx": 32, "bf16x2": 1}, "bottleneck": {"f16mx": 32, "bf16x2": 8}}


def branch_batched_default(kind, mx, n_images):
    """WSOVOD_BRANCH_BATCHED = 0 / 1 forces the loop / the one launch (A/B runs; read at every call), else the measured
    table of the block kind ("basic" / "bottleneck")."""
    env = os.environ.get("WSOVOD_BRANCH_BATCHED")
    if env in ("0", "1"):
        return env == "1"
    return n_images <= BATCHED_UP_TO[kind]["f16mx" if mx else "bf16x2"]


class _MRRPBlock:
    """What the two MRRP blocks share: the branch bookkeeping and the shortcut, evaluated once where the input is shared."""

    def _init_mrrp(self, num_branch, dilations, concat_output, test_branch_idx, shared_input, has_pool):
        dilations = tuple(int(d) for d in dilations)
        assert num_branch == len(dilations)
        if has_pool:
            raise NotImplementedError("wsovod_amd: the MRRP residual blocks are built for res5 (no pool; MODEL.MRRP.MRRP_STAGE)")
        if test_branch_idx != -1:
            raise NotImplementedError(f"wsovod_amd: MODEL.MRRP.TEST_BRANCH_IDX = {test_branch_idx}: every shipped MRRP config "
                                      "runs all branches (-1)")
        self.num_branch, self.dilations, self.concat_output = num_branch, dilations, concat_output
        self.test_branch_idx, self.shared_input = test_branch_idx, shared_input

    def _branched(self, x, conv, shared_input, **kw):
        """One conv of the block over all branches: the one-launch form where the table says so ("parity" / "parity_mx", whole
        32-value channel groups), else the loop over `hip_conv`."""
        n = x.shape[0] if shared_input else x.shape[0] // self.num_branch
        batched = H.x2_active() and conv.in_channels % 32 == 0 and conv.out_channels % 32 == 0 \
            and branch_batched_default(self.KIND, H.mx_of(x), n)
        return hip_conv_branches(x, conv, self.dilations, shared_input, batched=bool(batched), **kw)

    def _shortcut(self, x):
        """-> (the residual, whether it is ONE map for every branch)."""
        return (hip_conv(x, self.shortcut) if self.shortcut is not None else x), self.shared_input

    def forward(self, x):
        """x: block 0 of the stage (shared_input): the (N, H, W, Cin) NHWC map every branch reads; else (num_branch * N, H, W,
        Cin), branch-major -> (num_branch * N, H, W, Cout), branch-major."""
        return self.run(x)


class MRRPBasicBlock(_MRRPBlock, BasicBlock):
    """resnet_wsl_mrrp.py:122-239: both 3x3 convs once per branch dilation; `out_b + shortcut_b`, ReLU."""

    KIND = "basic"

    def __init__(self, in_channels, out_channels, *, stride=1, norm="BN", num_branch=3, dilations=(1, 2, 3), concat_output=False,
                 test_branch_idx=-1, has_pool=False, shared_input=False):
        BasicBlock.__init__(self, in_channels, out_channels, stride=stride, norm=norm, dilation=1, has_pool=has_pool)
        self._init_mrrp(num_branch, dilations, concat_output, test_branch_idx, shared_input, has_pool)

    def run(self, x, saving=False):
        assert not saving, "the MRRP stages are frozen"
        last = getattr(self, "_emits_fp32", False)
        h = self._branched(x, self.conv1, self.shared_input, relu=True)
        sc, sc_shared = self._shortcut(x)
        return self._branched(h, self.conv2, False, relu=True, out_fp32=last, residual=sc, residual_shared=sc_shared)


class MRRPBottleneckBlock(_MRRPBlock, BottleneckBlock):
    """resnet_wsl_mrrp.py:373-522: conv1 / conv3 ordinary 1x1 convs, conv2 (3x3) once per branch dilation."""

    KIND = "bottleneck"

    def __init__(self, in_channels, out_channels, *, bottleneck_channels, stride=1, num_groups=1, norm="BN", stride_in_1x1=False,
                 num_branch=3, dilations=(1, 2, 3), concat_output=False, test_branch_idx=-1, has_pool=False, shared_input=False):
        BottleneckBlock.__init__(self, in_channels, out_channels, bottleneck_channels=bottleneck_channels, stride=stride,
                                 num_groups=num_groups, norm=norm, stride_in_1x1=stride_in_1x1, dilation=1, has_pool=has_pool)
        self._init_mrrp(num_branch, dilations, concat_output, test_branch_idx, shared_input, has_pool)

    def run(self, x, saving=False):
        assert not saving, "the MRRP stages are frozen"
        last = getattr(self, "_emits_fp32", False)
        h = hip_conv(x, self.conv1, relu=True)  # shared input: ONCE for all branches; else over the num_branch * N maps
        h = self._branched(h, self.conv2, self.shared_input, relu=True)
        sc, sc_shared = self._shortcut(x)
        if sc_shared:  # block 0: the one shortcut map under every branch's conv3
            return self._branched(h, self.conv3, False, relu=True, out_fp32=last, residual=sc, residual_shared=True)
        return hip_conv(h, self.conv3, relu=True, residual=sc, out_fp32=last)


class MRRPResNet(ResNet):
    """resnet_wsl_mrrp.py:705-889 with res5 made of MRRP blocks."""

    def __init__(self, stem, stages, num_branch, branch_dilations, out_features=None, freeze_at=0, precision="bf16"):
        self.num_branch, self.branch_dilations = num_branch, tuple(int(d) for d in branch_dilations)
        super().__init__(stem, stages, out_features=out_features, freeze_at=freeze_at, precision=precision)

    @property
    def mrrp_stacked(self):
        """The output map is branch-major (res5 is an MRRP stage): MODEL.MRRP.MRRP_ON must be set for the heads."""
        return "res5" in self.stage_names

    @property
    def mrrp_num_branch(self):
        """Branches stacked along N in the output map."""
        return self.num_branch if self.mrrp_stacked else 1


@BACKBONE_REGISTRY.register()
def build_mrrp_wsl_resnet_backbone(cfg, input_shape):
    """resnet_wsl_mrrp.py:904-1027."""
    m, r = cfg.MODEL.MRRP, cfg.MODEL.RESNETS
    dilations = [int(d) for d in m.BRANCH_DILATIONS]
    if m.MRRP_STAGE != "res5":
        raise NotImplementedError(f"wsovod_amd: MODEL.MRRP.MRRP_STAGE = {m.MRRP_STAGE!r}: every shipped WSR MRRP config branches "
                                  "res5 (stride 1, no pool)")
    if m.TEST_BRANCH_IDX != -1:
        raise NotImplementedError(f"wsovod_amd: MODEL.MRRP.TEST_BRANCH_IDX = {m.TEST_BRANCH_IDX}: every shipped MRRP config sets "
                                  "-1 (all branches, in training and in testing)")
    if len(dilations) != m.NUM_BRANCH:
        raise NotImplementedError(f"wsovod_amd: MODEL.MRRP.BRANCH_DILATIONS = {dilations} does not name MODEL.MRRP.NUM_BRANCH = "
                                  f"{m.NUM_BRANCH} dilations")
    if m.NUM_BRANCH > MAX_BRANCHES:
        raise NotImplementedError(f"wsovod_amd: MODEL.MRRP.NUM_BRANCH = {m.NUM_BRANCH}: at most {MAX_BRANCHES} branches are built")
    if cfg.MODEL.BACKBONE.FREEZE_AT < 5:
        raise NotImplementedError(f"wsovod_amd: MODEL.BACKBONE.FREEZE_AT = {cfg.MODEL.BACKBONE.FREEZE_AT} with "
                                  "build_mrrp_wsl_resnet_backbone: the MRRP stages run forward-only (every shipped config "
                                  "freezes the backbone, FREEZE_AT 5)")
    if any(r.DEFORM_ON_PER_STAGE):
        raise NotImplementedError("wsovod_amd: MODEL.RESNETS.DEFORM_ON_PER_STAGE: deformable conv is not used by the WSR configs")
    if r.NUM_GROUPS != 1:
        raise NotImplementedError(f"wsovod_amd: MODEL.RESNETS.NUM_GROUPS = {r.NUM_GROUPS}: grouped convolution is not on the "
                                  "WSR hot path")

    def res5_as_mrrp(stage_idx, kargs):
        if stage_idx != 5:
            return
        nb = kargs["num_blocks"]
        kargs.pop("dilation")
        kargs["block_class"] = MRRPBasicBlock if kargs["block_class"] is BasicBlock else MRRPBottleneckBlock
        kargs.update(num_branch=m.NUM_BRANCH, dilations=dilations, test_branch_idx=m.TEST_BRANCH_IDX,
                     concat_output_per_block=[False] * (nb - 1) + [True], shared_input_per_block=[True] + [False] * (nb - 1))

    stem, stages = wsl_resnet_stem_and_stages(cfg, input_shape, stage_hook=res5_as_mrrp)
    return MRRPResNet(stem, stages, m.NUM_BRANCH, dilations, out_features=r.OUT_FEATURES, freeze_at=cfg.MODEL.BACKBONE.FREEZE_AT,
                      precision=forward_precision(cfg.MODEL.HIP.PRECISION))
