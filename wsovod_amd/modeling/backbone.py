"""WSL ResNet ("DC5", output stride 8) backbone on the HIP implicit-GEMM convolution.

Host-side mirror of the reference's wsovod/modeling/backbone/resnet_wsl.py: same classes (`BasicStem`, `BasicBlock`,
`BottleneckBlock`, `ResNet`, `build_wsl_resnet_backbone`), same constructor arguments, same parameter/buffer names (so
reference d2 checkpoints load), same `forward(x) -> {"res5": Tensor}` / `output_shape()` / `freeze()` surface.  The compute is
not torch: every conv (+ folded FrozenBN affine + ReLU + residual add) is one launch of the MFMA implicit-GEMM kernel over
NHWC activations, pools are the NHWC max-pool kernel.  The returned feature map is logically NCHW but stored NHWC
(torch.channels_last), which the ROIPooler reads directly.

This module holds the blocks, the stem, `FrozenForwardMixin` -- what the meta-arch and the trainers call on any backbone
(backbone_vgg.py, backbone_vgg_mrrp.py build on it) --, `ResNet`, the frozen forward as a HIP graph and the builder.

    conv.py            the parameter holders and weight folds, `hip_conv`, the first conv from the uint8 canvas, the ONE
                       forward of a residual block
    conv_backward.py   `_TrainableStage` / `_TrainableStem`: the backward of a trainable stage on the HIP kernels

Scope: every shipped WSR config freezes the whole backbone (FREEZE_AT: 5): the HIP kernels are the FORWARD of
every conv.  A trainable stage (FREEZE_AT < 5, resnet_wsl.py:530-552) runs its forward on those kernels and its BACKWARD too
(conv_backward.py).  Never a CPU path; tests/test_gpu_freeze_at.py pins it to the reference (G19), to the oracle
(FREEZE_AT = 0) and to the torch re-evaluation (FREEZE_AT 1 - 4).
"""
import os
import sys
import types
import warnings

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from ..config import BACKBONE_REGISTRY
from ..layers import hip_ops as H, mx_guard, precision as P
from ..structures import ShapeSpec
from . import conv, conv_backward
from .conv import (Conv2d, FrozenBatchNorm2d, ResidualBlock, c2_msra_fill, first_conv, get_norm,  # noqa: F401  (re-exported)
                   hip_conv)
from .conv_backward import (_TrainableStage, _TrainableStem, _block_backward, _block_forward_saving,  # noqa: F401  (re-exported:
                            _conv_dgrad, _conv_wgrad, _hip_backward_ok, _masked, _torch_block, _torch_conv)  # this module held them)

__all__ = ["BasicStem", "BasicBlock", "BottleneckBlock", "ResNet", "FrozenForwardMixin", "FrozenBatchNorm2d", "Conv2d",
           "build_wsl_resnet_backbone", "make_stage", "hip_conv", "forward_precision"]


def _forwarded(owner, name):
    return property(lambda module: getattr(owner, name), lambda module, value: setattr(owner, name, value))


class _Module(types.ModuleType):
    """The two limits that code lowers from outside lived in this module before conv.py / conv_backward.py took them.  A
    plain re-export would be a copy: lowered here, the owner would go on reading its own.  Here they are the owner's
    attribute itself, for reading and for setting."""

    CONV_MAX_OPERAND_BYTES = _forwarded(conv, "CONV_MAX_OPERAND_BYTES")
    WGRAD_PATCH_BYTES = _forwarded(conv_backward, "WGRAD_PATCH_BYTES")


sys.modules[__name__].__class__ = _Module


class CNNBlockBase(nn.Module):
    def __init__(self, in_channels, out_channels, stride):
        super().__init__()
        self.in_channels, self.out_channels, self.stride = in_channels, out_channels, stride

    def freeze(self):
        for p in self.parameters():
            p.requires_grad = False
        return self


class BasicBlock(CNNBlockBase, ResidualBlock):
    """resnet_wsl.py:24-110: two 3x3 convs; the block stride lives in the trailing max pool."""

    def __init__(self, in_channels, out_channels, *, stride=1, norm="BN", dilation=1, has_pool=False):
        super().__init__(in_channels, out_channels, stride)
        self._init_pool(has_pool, stride)
        stride = 1
        if in_channels != out_channels:
            self.shortcut = Conv2d(in_channels, out_channels, 1, stride=stride, bias=False,
                                   norm=get_norm(norm, out_channels))
        else:
            self.shortcut = None
        self.conv1 = Conv2d(in_channels, out_channels, 3, stride=stride, padding=dilation, dilation=dilation,
                            bias=False, norm=get_norm(norm, out_channels))
        self.conv2 = Conv2d(out_channels, out_channels, 3, stride=1, padding=dilation, dilation=dilation,
                            bias=False, norm=get_norm(norm, out_channels))
        for layer in [self.conv1, self.conv2, self.shortcut]:
            if layer is not None:
                c2_msra_fill(layer)

    def convs(self):
        return [self.conv1, self.conv2]

    def forward(self, x):
        return self.run(x)


class BottleneckBlock(CNNBlockBase, ResidualBlock):
    """resnet_wsl.py:113-241: 1x1 -> 3x3 (dilated) -> 1x1 + shortcut."""

    def __init__(self, in_channels, out_channels, *, bottleneck_channels, stride=1, num_groups=1, norm="BN",
                 stride_in_1x1=False, dilation=1, has_pool=False):
        super().__init__(in_channels, out_channels, stride)
        if num_groups != 1:
            raise NotImplementedError("grouped convolution is not on the WSR hot path")
        self._init_pool(has_pool, stride)
        stride = 1
        if in_channels != out_channels:
            self.shortcut = Conv2d(in_channels, out_channels, 1, stride=stride, bias=False,
                                   norm=get_norm(norm, out_channels))
        else:
            self.shortcut = None
        stride_1x1, stride_3x3 = (stride, 1) if stride_in_1x1 else (1, stride)
        self.conv1 = Conv2d(in_channels, bottleneck_channels, 1, stride=stride_1x1, bias=False,
                            norm=get_norm(norm, bottleneck_channels))
        self.conv2 = Conv2d(bottleneck_channels, bottleneck_channels, 3, stride=stride_3x3, padding=dilation,
                            dilation=dilation, bias=False, norm=get_norm(norm, bottleneck_channels))
        self.conv3 = Conv2d(bottleneck_channels, out_channels, 1, bias=False, norm=get_norm(norm, out_channels))
        for layer in [self.conv1, self.conv2, self.conv3, self.shortcut]:
            if layer is not None:
                c2_msra_fill(layer)

    def convs(self):
        return [self.conv1, self.conv2, self.conv3]

    def forward(self, x):
        return self.run(x)


class BasicStem(CNNBlockBase):
    """resnet_wsl.py:361-421: conv3x3 s2 -> conv3x3 -> conv3x3 -> maxpool k2 s2 (stride 4)."""

    def __init__(self, in_channels=3, out_channels=64, norm="BN"):
        super().__init__(in_channels, out_channels, 4)
        self.conv1 = Conv2d(in_channels, out_channels, 3, stride=2, padding=1, bias=False,
                            norm=get_norm(norm, out_channels))
        self.conv2 = Conv2d(out_channels, out_channels, 3, stride=1, padding=1, bias=False,
                            norm=get_norm(norm, out_channels))
        self.conv3 = Conv2d(out_channels, out_channels, 3, stride=1, padding=1, bias=False,
                            norm=get_norm(norm, out_channels))
        for c in (self.conv1, self.conv2, self.conv3):
            c2_msra_fill(c)

    def _tail(self, x):
        x = hip_conv(x, self.conv2, relu=True)
        return hip_conv(x, self.conv3, relu=True, pool2=True)

    def forward(self, x):
        """x: NHWC with Cin zero-padded to the kernel's K-step (generic float entry)."""
        return self._tail(hip_conv(x, self.conv1, relu=True))

    def forward_uint8(self, images_u8, sizes, pixel_mean, pixel_std, compute_dtype):
        """The stem from the uint8 canvas (conv.py: first_conv)."""
        return self._tail(first_conv(self.conv1, images_u8, sizes, pixel_mean, pixel_std, 2, compute_dtype))


def forward_precision(name):
    """The precision every module sees (layers/precision.py:TABLE); the meta-arch enters a composite name's flags."""
    return P.of(name).forward


_WARNED_TRAINABLE = set()


def _warn_trainable_stage_once(name):
    if name not in _WARNED_TRAINABLE:
        _WARNED_TRAINABLE.add(name)
        warnings.warn(f"wsovod_amd: backbone stage {name} is trainable (MODEL.BACKBONE.FREEZE_AT < 5): the step leaves the "
                      "optimised path -- no frozen-forward overlap, no step graph, no backbone graph; its backward runs on "
                      "the HIP kernels too (the bf16x3 modes: a torch re-evaluation of the stage; DESIGN.md section 7)",
                      stacklevel=3)


class FrozenForwardMixin:
    """What the meta-arch and the trainers call on a backbone, shared by `ResNet` and `VGG16` (backbone_vgg.py): the fused
    uint8 entry with its precision mode, the frozen forward as a HIP graph, the parameter walks cached per module tree.  The
    class provides `precision`, `_forward_uint8(images_u8, sizes, mean, std)`, `has_trainable_stage` and the
    `_out_feature_{channels,strides}` / `_out_features` tables."""

    @property
    def compute_dtype(self):
        return P.of(self.precision).compute_dtype

    def _emit_fp32_from(self, block):
        """"parity": bf16x2 maps inside, real fp32 from `block` -- the last one -- for the one map that leaves the backbone."""
        if P.is_x2(P.of(self.precision).x3):
            if list(self._out_features) != [self.stage_names[-1]]:
                raise NotImplementedError('MODEL.HIP.PRECISION "parity" returns the last stage only (bf16x2 maps inside)')
            block._emits_fp32 = True

    def _float_entry(self, x):
        """(N,C,H,W) normalised float images -> (NHWC in the compute dtype, Cin 3 padded to one K-step; the entry's mode)."""
        cd, x3 = self.compute_dtype, P.of(self.precision).x3_float_entry
        kstep = 64 if (cd == torch.bfloat16 or x3) else 32
        with torch.no_grad():
            xn = x.permute(0, 2, 3, 1).to(cd)
            xn = F.pad(xn, (0, kstep - xn.size(-1))).contiguous()
        return xn, H.x3_mode(x3)

    MX_MIN_TILES = int(os.environ.get("WSOVOD_MX_MIN_TILES", "200"))  # "parity_mx": fewest tiles of the f16mx kernel's ONE shape

    MX_FIRST = None  # name of the earliest stage the f16mx run may start at (None: any)

    def _mx_block_ok(self, block):
        """Whether `block` may run on the f16mx kernels (the backbone's own rule)."""
        raise NotImplementedError

    def _mx_from(self):
        """"parity_mx": index of the first stage that runs on the f16mx kernels -- the trailing run of FROZEN stages, from
        MX_FIRST on, whose every block passes `_mx_block_ok`; len(stages) = none."""
        first = len(self.stages)
        floor = self.stage_names.index(self.MX_FIRST) if self.MX_FIRST is not None else 0
        for i in range(len(self.stages) - 1, floor - 1, -1):
            stage = self.stages[i]
            if not all(self._mx_block_ok(b) for b in stage.children()) \
                    or any(p.requires_grad for p in self._stage_params(stage)):
                break
            first = i
        return first

    def _mx_first_stage(self):
        return self._mx_from() if (H.mx_active() and list(self._out_features) == [self.stage_names[-1]]) else len(self.stages)

    def _mx_min_tiles(self, x, first):
        """256-row tiles of the smallest conv of the f16mx run that starts with the map x."""
        return -(-(x.shape[0] * x.shape[1] * x.shape[2]) // 256)

    def _cross_to_mx(self, x, si, mx_from):
        """Ahead of stage `si`: the map that crosses from the bf16x2 layers to the f16mx ones (enough tiles: see above)."""
        if si == mx_from and si > 0 and self._mx_min_tiles(x, si) >= self.MX_MIN_TILES:
            with torch.no_grad():
                x = H.mx_from_x2(x)
                mx_guard.audit("backbone.mx_from_x2", x)
        return x

    def _param_list(self):
        cached = getattr(self, "_params_cache", None)
        if cached is None:  # the module tree is fixed after construction: walk it once, not every step
            cached = self._params_cache = list(self.parameters())
        return cached

    def _stage_params(self, stage):
        cache = self.__dict__.setdefault("_stage_params_cache", {})
        got = cache.get(id(stage))
        if got is None:  # (fixed after construction, as _param_list)
            got = cache[id(stage)] = list(stage.parameters())
        return got

    def forward_uint8(self, images_u8, sizes, pixel_mean, pixel_std, allow_graph=False):
        """Fused entry used by the meta-arch: uint8 canvas -> normalise + im2col -> stem conv1 GEMM.
        allow_graph: the caller consumes the maps before its next call with this shape (the training step's frozen
        forward): small batches may then come from a captured HIP graph, whose outputs are that graph's STATIC buffers
        -- overwritten by the next replay.  inference() / TTA keep the eager launches (fresh tensors)."""
        with H.x3_mode(P.of(self.precision).x3):
            if allow_graph and self.graph_max_batch and images_u8.is_cuda and images_u8.size(0) <= self.graph_max_batch \
                    and not self.has_trainable_stage:
                g = self._graph_for(images_u8, sizes, pixel_mean, pixel_std)
                if g is not None:
                    return g(images_u8)
            return self._forward_uint8(images_u8, sizes, pixel_mean, pixel_std)

    # ---- the frozen forward as a HIP graph (small batches: the ~25 launches of the backbone cost more host time than
    # device time; one replay instead).  Opt-in (`graph_max_batch`, set by the overlapped trainer): the returned maps
    # are the graph's static buffers, valid until the next call with the same input shape ----
    graph_max_batch = 0
    GRAPH_CACHE = 4  # graphs kept (each holds the backbone's activations of its shape)
    GRAPH_AFTER = 3  # calls with a shape before it is captured

    def _graph_fingerprint(self):
        ps = getattr(self, "_graph_tensors", None)
        if ps is None:
            ps = self._graph_tensors = list(self.parameters()) + list(self.buffers())
        return sum(t._version for t in ps), ps[0].data_ptr() if ps else 0

    def _graph_for(self, images_u8, sizes, pixel_mean, pixel_std):
        from .._lib import PROFILING

        if PROFILING[0] or torch.cuda.is_current_stream_capturing():
            return None
        fp = self._graph_fingerprint()
        cache = self.__dict__.setdefault("_graphs", {})
        if any(v and v.fingerprint != fp for v in cache.values()):
            cache.clear()  # a weight changed (load_state_dict, broadcast): the folded copies the graphs point at are stale
        key = (tuple(images_u8.shape), sizes.data_ptr(), tuple(pixel_mean), tuple(pixel_std), H.x3_active(), H.mx_active())
        g = cache.get(key)
        if g is None:
            # capture on the third call with a shape: with multi-scale inputs most shapes never repeat, and a capture
            # costs three forwards
            seen = self.__dict__.setdefault("_graph_seen", {})
            if len(seen) > 64:
                seen.clear()
            seen[key] = seen.get(key, 0) + 1
            if seen[key] < self.GRAPH_AFTER:
                return None
            if len(cache) >= self.GRAPH_CACHE:
                cache.pop(next(iter(cache)))
            try:
                g = _BackboneGraph(self, images_u8, sizes, pixel_mean, pixel_std, fp)
            except Exception as e:  # noqa: BLE001 -- out of memory in the graph's pool, an API call refused under capture
                import warnings

                warnings.warn(f"wsovod_amd: HIP graph capture of the frozen backbone failed for input shape "
                              f"{tuple(images_u8.shape)} ({type(e).__name__}: {e}); this shape keeps the eager launches")
                g = False  # remembered: never retried for this key
            cache[key] = g
        return g or None

    size_divisibility = 0

    def output_shape(self):
        return {name: ShapeSpec(channels=self._out_feature_channels[name], stride=self._out_feature_strides[name])
                for name in self._out_features}


class ResNet(FrozenForwardMixin, nn.Module):
    """resnet_wsl.py:424-607."""

    def __init__(self, stem, stages, num_classes=None, out_features=None, freeze_at=0, precision="bf16"):
        super().__init__()
        if num_classes is not None:
            raise NotImplementedError("classification head is not on the detection hot path")
        self.stem = stem
        self.num_classes = num_classes
        self.precision = precision
        current_stride = self.stem.stride
        self._out_feature_strides = {"stem": current_stride}
        self._out_feature_channels = {"stem": self.stem.out_channels}
        self.stage_names, self.stages = [], []
        if out_features is not None:
            num_stages = max([{"res2": 1, "res3": 2, "res4": 3, "res5": 4}.get(f, 0) for f in out_features])
            stages = stages[:num_stages]
        for i, blocks in enumerate(stages):
            assert len(blocks) > 0, len(blocks)
            name = "res" + str(i + 2)
            stage = nn.Sequential(*blocks)
            self.add_module(name, stage)
            self.stage_names.append(name)
            self.stages.append(stage)
            self._out_feature_strides[name] = current_stride = int(
                current_stride * np.prod([k.stride for k in blocks]))
            self._out_feature_channels[name] = blocks[-1].out_channels
        self.stage_names = tuple(self.stage_names)
        if out_features is None:
            out_features = [name]
        self._out_features = out_features
        assert len(self._out_features)
        self._emit_fp32_from(list(self.stages[-1].children())[-1])
        children = [x[0] for x in self.named_children()]
        for out_feature in self._out_features:
            assert out_feature in children, "Available children: {}".format(", ".join(children))
        self.freeze(freeze_at)

    def _check_frozen(self):
        """The generic float entry (`forward(x)`, a normalised float image) has no trainable-stem path: the stem's first conv
        trains through the fused uint8 entry (`forward_uint8`, what the meta-arch calls; _TrainableStem)."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.stem.parameters()):
            raise NotImplementedError(
                "wsovod_amd: MODEL.BACKBONE.FREEZE_AT = 0 (a trainable stem) trains through ResNet.forward_uint8 (the uint8 "
                "entry the meta-arch uses); the float entry ResNet.forward(x) runs the stem forward-only")

    @property
    def has_trainable_stage(self):
        """True when a residual stage is trainable (FREEZE_AT < 5): the backbone forward then reads weights the optimizer
        updates, and the trainers may no longer run it ahead of the previous step's update."""
        return any(p.requires_grad for p in self._param_list())

    def _mx_block_ok(self, b):
        """"parity_mx" (FrozenForwardMixin._mx_from): residual blocks without pools whose convs are at least 256 channels wide,
        whole 32-value groups, stride 1, a 1x1 / stride-1 shortcut (res4 / res5 of WSR_18: what the numerics gate covered,
        profiles/r06_mx_gate.md; the BottleneckBlocks of WSR_50's res4 / res5 -- 1x1 / 3x3 / 1x1, 256 - 2048 channels -- are the
        same contractions and take the same kernel: tests/test_gpu_full_size.py holds them to the same bar).  The f16mx kernel
        has ONE tile shape (256 x 256, a workgroup per CU): below ~200 tiles per conv (fewer than 8 images of 800 x 600) the
        bf16x2 path's smaller tiles / split-K forms win and the stages stay on it (MX_MIN_TILES) -- same precision mode, same
        bound (both formats were gated alone and together)."""
        if not isinstance(b, ResidualBlock) or b.has_pool:
            return False
        return (all(c.in_channels % 32 == 0 and c.out_channels % 32 == 0 and c.out_channels >= 256 and c.stride == 1
                    for c in b.convs())
                and (b.shortcut is None or (b.shortcut.kernel_size == 1 and b.shortcut.stride == 1)))

    def _run(self, x):
        outputs = {}
        if "stem" in self._out_features:
            outputs["stem"] = x.permute(0, 3, 1, 2)
        mx_from = self._mx_first_stage()
        for si, (name, stage) in enumerate(zip(self.stage_names, self.stages)):
            params = self._stage_params(stage)
            x = self._cross_to_mx(x, si, mx_from)
            if torch.is_grad_enabled() and any(p.requires_grad for p in params):
                _warn_trainable_stage_once(name)
                x = _TrainableStage.apply(stage, H.x3_active(), x, *params)
            else:
                with torch.no_grad():
                    x = stage(x)
            if name in self._out_features:
                outputs[name] = x.permute(0, 3, 1, 2)  # logical NCHW, NHWC memory (channels_last)
        return outputs

    def forward(self, x):
        """x: (N,C,H,W) normalised float image batch -> {name: (N,C',H/8,W/8) channels_last}."""
        assert x.dim() == 4, f"ResNet takes an input of shape (N, C, H, W). Got {x.shape} instead!"
        self._check_frozen()
        xn, mode = self._float_entry(x)
        with mode:
            with torch.no_grad():
                xs = self.stem(xn)
            return self._run(xs)

    def _stem_conv1(self, images_u8, sizes, pixel_mean, pixel_std):
        """relu(conv1 (normalised image)) as the stem's forward produces it."""
        return first_conv(self.stem.conv1, images_u8, sizes, pixel_mean, pixel_std, 2, self.compute_dtype)

    def _stem_uint8(self, images_u8, sizes, pixel_mean, pixel_std):
        return self.stem.forward_uint8(images_u8, sizes, pixel_mean, pixel_std, self.compute_dtype)

    def _forward_uint8(self, images_u8, sizes, pixel_mean, pixel_std):
        stem_params = self._stage_params(self.stem)
        if torch.is_grad_enabled() and any(p.requires_grad for p in stem_params):
            # MODEL.BACKBONE.FREEZE_AT = 0: the stem trains too (its backward on the HIP kernels, _TrainableStem)
            x3 = H.x3_active()
            if x3 in ("full", "fwd") or not (self.stem.out_channels == 64 and self.stem.in_channels == 3):
                raise NotImplementedError("wsovod_amd: MODEL.BACKBONE.FREEZE_AT = 0 (a trainable stem) is supported in the "
                                          "bf16 / fp32 / parity precisions on the 3 -> 64 stem")
            _warn_trainable_stage_once("stem")
            xs = _TrainableStem.apply(self, x3, images_u8, sizes, pixel_mean, pixel_std, *stem_params)
        else:
            with torch.no_grad():
                xs = self._stem_uint8(images_u8, sizes, pixel_mean, pixel_std)
        return self._run(xs)

    def freeze(self, freeze_at=0):
        if freeze_at >= 1:
            self.stem.freeze()
        for idx, stage in enumerate(self.stages, start=2):
            if freeze_at >= idx:
                for block in stage.children():
                    block.freeze()
        return self

    @staticmethod
    def make_stage(block_class, num_blocks, *, in_channels, out_channels, **kwargs):
        blocks = []
        for i in range(num_blocks):
            curr_kwargs = {}
            for k, v in kwargs.items():
                if k.endswith("_per_block"):
                    assert len(v) == num_blocks
                    curr_kwargs[k[: -len("_per_block")]] = v[i]
                else:
                    curr_kwargs[k] = v
            blocks.append(block_class(in_channels=in_channels, out_channels=out_channels, **curr_kwargs))
            in_channels = out_channels
        return blocks


class _BackboneGraph:
    """One captured frozen forward for one input shape: static input / output buffers, replayed per call."""

    def __init__(self, net, images_u8, sizes, pixel_mean, pixel_std, fingerprint):
        self.fingerprint = fingerprint
        self.sizes = sizes  # (kept alive: the kernels of the graph read it)
        self.static_in = torch.empty_like(images_u8)
        self.static_in.copy_(images_u8)
        main = torch.cuda.current_stream(images_u8.device)
        side = torch.cuda.Stream(device=images_u8.device)
        side.wait_stream(main)
        with torch.cuda.stream(side):  # warm-up outside the capture: weight folds, function attributes, allocator
            for _ in range(2):
                net._forward_uint8(self.static_in, sizes, pixel_mean, pixel_std)
        main.wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        # thread_local: a HIP call from another thread (a DataLoader's pin-memory thread, an eval thread) during the
        # capture -- it happens mid-training, on the third sighting of a shape -- must not abort it
        import gc

        gc_was_on = gc.isenabled()  # (no cyclic collection inside a capture: see engine/trainer.py:_StepGraph._capture)
        gc.disable()
        try:
            with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                self.out = net._forward_uint8(self.static_in, sizes, pixel_mean, pixel_std)
        finally:
            if gc_was_on:
                gc.enable()

    def __call__(self, images_u8):
        if images_u8.data_ptr() != self.static_in.data_ptr():
            self.static_in.copy_(images_u8)
        self.graph.replay()
        return self.out


def make_stage(*args, **kwargs):
    return ResNet.make_stage(*args, **kwargs)


def wsl_resnet_stem_and_stages(cfg, input_shape, stage_hook=None):
    """resnet_wsl.py:623-707 (stage wiring: stride-by-maxpool, dilated res4/res5) -> (stem, [blocks of res2 .. res5]).
    stage_hook(stage_idx, stage_kargs): may rewrite the `make_stage` arguments of a stage (backbone_resnet_mrrp.py)."""
    norm = cfg.MODEL.RESNETS.NORM
    stem = BasicStem(in_channels=input_shape.channels, out_channels=cfg.MODEL.RESNETS.STEM_OUT_CHANNELS, norm=norm)
    depth = cfg.MODEL.RESNETS.DEPTH
    num_groups = cfg.MODEL.RESNETS.NUM_GROUPS
    width_per_group = cfg.MODEL.RESNETS.WIDTH_PER_GROUP
    bottleneck_channels = num_groups * width_per_group
    in_channels = cfg.MODEL.RESNETS.STEM_OUT_CHANNELS
    out_channels = cfg.MODEL.RESNETS.RES2_OUT_CHANNELS
    stride_in_1x1 = cfg.MODEL.RESNETS.STRIDE_IN_1X1
    res5_dilation = cfg.MODEL.RESNETS.RES5_DILATION
    assert res5_dilation in {1, 2}, "res5_dilation cannot be {}.".format(res5_dilation)
    if any(cfg.MODEL.RESNETS.DEFORM_ON_PER_STAGE):
        raise NotImplementedError("deformable conv is not used by the WSR configs")
    num_blocks_per_stage = {18: [2, 2, 2, 2], 34: [3, 4, 6, 3], 50: [3, 4, 6, 3], 101: [3, 4, 23, 3],
                            152: [3, 8, 36, 3]}[depth]
    if depth in [18, 34]:
        assert out_channels == 64, "Must set MODEL.RESNETS.RES2_OUT_CHANNELS = 64 for R18/R34"
        assert num_groups == 1, "Must set MODEL.RESNETS.NUM_GROUPS = 1 for R18/R34"
    stages = []
    for idx, stage_idx in enumerate(range(2, 6)):
        dilation = res5_dilation if stage_idx == 5 or stage_idx == 4 else 1
        first_stride = 2 if idx == 0 or (stage_idx == 3 and res5_dilation == 1) else 1
        has_pool = stage_idx == 2 or stage_idx == 3
        nb = num_blocks_per_stage[idx]
        stage_kargs = {"num_blocks": nb, "stride_per_block": [1] * (nb - 1) + [first_stride],
                       "has_pool_per_block": [False] * (nb - 1) + [has_pool], "in_channels": in_channels,
                       "out_channels": out_channels, "norm": norm, "dilation": dilation}
        if depth in [18, 34]:
            stage_kargs["block_class"] = BasicBlock
        else:
            stage_kargs.update(block_class=BottleneckBlock, bottleneck_channels=bottleneck_channels,
                               stride_in_1x1=stride_in_1x1, num_groups=num_groups)
        if stage_hook is not None:
            stage_hook(stage_idx, stage_kargs)
        stages.append(ResNet.make_stage(**stage_kargs))
        in_channels = out_channels
        out_channels *= 2
        bottleneck_channels *= 2
    return stem, stages


@BACKBONE_REGISTRY.register()
def build_wsl_resnet_backbone(cfg, input_shape):
    """resnet_wsl.py:623-707."""
    stem, stages = wsl_resnet_stem_and_stages(cfg, input_shape)
    return ResNet(stem, stages, out_features=cfg.MODEL.RESNETS.OUT_FEATURES, freeze_at=cfg.MODEL.BACKBONE.FREEZE_AT,
                  precision=forward_precision(cfg.MODEL.HIP.PRECISION))
