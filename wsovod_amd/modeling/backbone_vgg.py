"""VGG16 "DC5" backbone (the reference's V_16 configs) on the HIP implicit-GEMM convolution.

Host-side mirror of wsovod/modeling/backbone/vgg.py: `PlainBlock`, `VGG16`, `build_vgg_backbone` with the reference's surface
-- stages `plain1 .. plain5`, each an `nn.Sequential` of one block, state-dict keys `plain{i}.0.conv{j}.{weight,bias}` (the
reference's d2 checkpoints load), `output_shape()` strides 2 / 4 / 8 / 8 / 8 (16 / 16 undilated), `_out_features = ["plain5"]`,
`freeze()` per block.  Every conv is 3x3, stride 1, with a bias and no norm, followed by ReLU; the strides live in the
stages' trailing max pools: MaxPool2d(2, 2), and -- with CONV5_DILATION = 2 -- MaxPool2d(2, stride=1, padding=0) after plain4,
which shrinks the map by one row and one column (vgg.py:98-99,181-184).

Forward only: every shipped V_16 config freezes the whole backbone (FREEZE_AT: 5), and a trainable plain stage raises.

    plain1   conv1_1 from the uint8 canvas by conv.py's first_conv at stride 1 (csrc/stem.hip: wsovod_stem_conv1_s1[_x2]; the
             fp32 / bf16x3 precisions: wsovod_stem_im2col_ex + GEMM); conv1_2 + its pool in ONE launch of the 64-channel kernel
             (the pool in its epilogue): the full-resolution 64-channel map is written once and read once
    plain2-5 hip_conv per conv (conv.py), the NHWC pool kernel per stage
    parity   bf16x2 maps inside, real fp32 from the last conv of plain5
    parity_mx  the trailing run of stages whose convs are >= 256 wide (plain3 on) on the f16mx kernels: the crossing is
             mx_from_x2 on the run's input, the pools inside the run are the f16mx pool (wsovod_maxpool2x2_nhwc with
             WSOVOD_F16MX: the winner's three fields copied verbatim)
"""
import torch
from torch import nn

from ..config import BACKBONE_REGISTRY
from ..layers import hip_ops as H, mx_guard
from .backbone import CNNBlockBase, FrozenForwardMixin, forward_precision
from .conv import Conv2d, c2_msra_fill, first_conv, hip_conv

__all__ = ["PlainBlock", "VGG16", "build_vgg_backbone"]


class PlainBlock(CNNBlockBase):
    """vgg.py:34-121: `num_conv` 3x3 convs (bias, no norm) + ReLU each, then an optional MaxPool2d(2, stride, padding=0)."""

    def __init__(self, in_channels, out_channels, num_conv=3, dilation=1, stride=1, has_pool=False):
        super().__init__(in_channels, out_channels, stride)
        assert 2 <= num_conv < 5
        self.num_conv, self.dilation = num_conv, dilation
        self.has_pool, self.pool_stride = has_pool, stride
        for j in range(num_conv):
            conv = Conv2d(in_channels if j == 0 else out_channels, out_channels, 3, stride=1, padding=dilation,
                          dilation=dilation, bias=True, norm=None)
            c2_msra_fill(conv)
            setattr(self, f"conv{j + 1}", conv)

    def convs(self):
        return [getattr(self, f"conv{j + 1}") for j in range(self.num_conv)]

    def _pool(self, x):
        """MaxPool2d(2, stride, padding=0): odd sizes floor; stride 1 gives (H - 1, W - 1)."""
        mx = H.mx_of(x)
        out = H.maxpool2x2_nhwc(x, self.pool_stride, zero_pad_br=False, x2=H.x2_active() and not mx, mx=mx)
        if mx:
            mx_guard.audit(self, out)  # (copied fields: in range when the producer's were; audited as every f16mx producer is)
        return out

    def forward(self, x, skip_first=False):
        """x: the block's NHWC input -- or, with skip_first, relu(conv1(input)) as the fused first-conv kernel left it."""
        convs = self.convs()[1 if skip_first else 0:]
        for j, conv in enumerate(convs):
            if j < len(convs) - 1:
                x = hip_conv(x, conv, relu=True)
            elif self.has_pool and self.pool_stride == 2 and not H.mx_of(x):
                # MaxPool2d(2, 2) rides in hip_conv: in the 64-channel kernel's epilogue (plain1), else the pool kernel
                return hip_conv(x, conv, relu=True, pool2=True)
            else:
                x = hip_conv(x, conv, relu=True, out_fp32=getattr(self, "_emits_fp32", False) and not self.has_pool)
        return self._pool(x) if self.has_pool else x


class VGG16(FrozenForwardMixin, nn.Module):
    """vgg.py:124-230."""

    has_trainable_stage = False

    def __init__(self, conv5_dilation, freeze_at, num_classes=None, out_features=None, precision="bf16"):
        super().__init__()
        if num_classes is not None:
            raise NotImplementedError("classification head is not on the detection hot path")
        if conv5_dilation not in (1, 2):
            raise ValueError(f"MODEL.VGG.CONV5_DILATION must be 1 or 2, got {conv5_dilation}")
        if freeze_at < 5:
            raise NotImplementedError(
                f"wsovod_amd: the VGG16 backbone is forward-only (MODEL.BACKBONE.FREEZE_AT = 5, as in every shipped V_16 "
                f"config); got FREEZE_AT = {freeze_at}: trainable plain stages are not built")
        self.num_classes, self.precision, self.conv5_dilation = num_classes, precision, conv5_dilation
        d = conv5_dilation
        s8 = 8 if d == 2 else 16
        plan = [  # (name, block arguments, output stride)
            ("plain1", dict(in_channels=3, out_channels=64, num_conv=2, stride=2, has_pool=True), 2),
            ("plain2", dict(in_channels=64, out_channels=128, num_conv=2, stride=2, has_pool=True), 4),
            ("plain3", dict(in_channels=128, out_channels=256, num_conv=3, stride=2, has_pool=True), 8),
            ("plain4", dict(in_channels=256, out_channels=512, num_conv=3, stride=1 if d == 2 else 2, has_pool=True), s8),
            ("plain5", dict(in_channels=512, out_channels=512, num_conv=3, stride=1, dilation=d, has_pool=False), s8),
        ]
        self._out_feature_strides, self._out_feature_channels = {}, {}
        self.stage_names, self.stages = [], []
        for name, kw, stride in plan:
            stage = nn.Sequential(self._make_block(name, kw))
            self.add_module(name, stage)
            self.stage_names.append(name)
            self.stages.append(stage)
            self._out_feature_strides[name] = stride
            self._out_feature_channels[name] = kw["out_channels"]
        self.stage_names = tuple(self.stage_names)
        if out_features is None:
            out_features = [name]
        self._out_features = out_features
        assert len(self._out_features)
        for f in self._out_features:
            assert f in self.stage_names, "Available children: {}".format(", ".join(self.stage_names))
        self._emit_fp32_from(self.stages[-1][0])
        self.freeze(freeze_at)

    def _make_block(self, name, kw):
        """The one block of stage `name` (backbone_vgg_mrrp.py: the MRRP plain5)."""
        return PlainBlock(**kw)

    def freeze(self, freeze_at=0):
        for idx, stage in enumerate(self.stages, start=1):
            if freeze_at >= idx:
                for block in stage.children():
                    block.freeze()
        return self

    # ---- "parity_mx" ----
    MX_FIRST = "plain3"  # the earliest stage the f16mx run may start at (the 1e-3 logit bar holds from here)

    def _mx_block_ok(self, b):
        """FrozenForwardMixin._mx_from: every conv at least 256 channels wide with whole 32-value channel groups (plain3 on)."""
        return all(c.in_channels % 32 == 0 and c.out_channels % 32 == 0 and c.out_channels >= 256 for c in b.convs())

    def _mx_min_tiles(self, x, first):
        """256-row tiles of the SMALLEST conv of the f16mx run that starts with the map x (its pools shrink the later ones)."""
        n, h, w = x.shape[:3]
        rows = n * h * w
        for stage in self.stages[first:]:
            for b in stage.children():
                rows = min(rows, n * h * w)
                if b.has_pool:
                    h, w = ((h - 2) // 2 + 1, (w - 2) // 2 + 1) if b.pool_stride == 2 else (h - 1, w - 1)
        return -(-rows // 256)

    def _run(self, x, first_stage_done=False):
        """x: the NHWC input of plain1 -- or, with first_stage_done, plain1's output."""
        outputs = {}
        mx_from = self._mx_first_stage()
        with torch.no_grad():
            for si, (name, stage) in enumerate(zip(self.stage_names, self.stages)):
                x = self._cross_to_mx(x, si, mx_from)
                if not (si == 0 and first_stage_done):
                    x = stage(x)
                if name in self._out_features:
                    outputs[name] = x.permute(0, 3, 1, 2)  # logical NCHW, NHWC memory (channels_last)
        return outputs

    def forward(self, x):
        """x: (N,C,H,W) normalised float image batch -> {name: (N,C',H',W') channels_last}."""
        assert x.dim() == 4, f"VGG16 takes an input of shape (N, C, H, W). Got {x.shape} instead!"
        xn, mode = self._float_entry(x)
        with mode:
            return self._run(xn)

    def _conv1_1(self, images_u8, sizes, pixel_mean, pixel_std):
        """relu(conv1_1(normalised image)): (N, Hp, Wp, 64) NHWC in the precision's activation format."""
        return first_conv(self.stages[0][0].conv1, images_u8, sizes, pixel_mean, pixel_std, 1, self.compute_dtype)

    def _forward_uint8(self, images_u8, sizes, pixel_mean, pixel_std):
        with torch.no_grad():
            x = self._conv1_1(images_u8, sizes, pixel_mean, pixel_std)
            x = self.stages[0][0](x, skip_first=True)
        return self._run(x, first_stage_done=True)


@BACKBONE_REGISTRY.register()
def build_vgg_backbone(cfg, input_shape):
    """vgg.py:233-243."""
    depth = cfg.MODEL.VGG.DEPTH
    if depth != 16:
        raise NotImplementedError(f"wsovod_amd: MODEL.VGG.DEPTH = {depth}: VGG16 is the only depth the reference builds")
    if input_shape.channels != 3:
        raise NotImplementedError("the VGG16 backbone takes 3-channel images")
    return VGG16(cfg.MODEL.VGG.CONV5_DILATION, cfg.MODEL.BACKBONE.FREEZE_AT,
                 precision=forward_precision(cfg.MODEL.HIP.PRECISION))
