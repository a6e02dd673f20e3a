"""GeneralizedRCNN_WSOVOD on the HIP hot path.

Mirror of /root/reference/wsovod/modeling/meta_arch/rcnn_wsovod.py:27-344: same registry name,
`forward(batched_inputs) -> dict[str, loss]` in training / `inference(...)` in eval, same
`batched_inputs` format (`image` uint8 CHW BGR, `instances`, `proposals`, `height`/`width`), same
sub-module names (`backbone`, `data_aware_head`, `roi_heads`) so state dicts are interchangeable.
The proposals-only branch (rcnn_wsovod.py:198-204) is the hot path; an RPN
(`MODEL.PROPOSAL_GENERATOR.NAME != "PrecomputedProposals"`) is a SURVEY 8f "next" row.
"""
import contextlib
import logging
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from torch import nn

from ..config import BACKBONE_REGISTRY, META_ARCH_REGISTRY, configurable
from ..layers import hip_ops as H
from ..layers import mx_guard, operand_cache, precision as P
from ..structures import Boxes, ImageList, Instances, ShapeSpec
from .class_heads import DataAwareFeaturesHead
from .fast_rcnn_open_vocabulary import segment_offsets
from .proposal_generator import build_proposal_generator
from .roi_heads import build_roi_heads

__all__ = ["GeneralizedRCNN_WSOVOD", "GeneralizedRCNN_WSOVOD_MixedDatasets", "build_model", "build_backbone"]


def build_backbone(cfg, input_shape=None):
    if input_shape is None:
        input_shape = ShapeSpec(channels=len(cfg.MODEL.PIXEL_MEAN))
    return BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg, input_shape)


def build_model(cfg):
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE)(cfg)
    model.to(torch.device(cfg.MODEL.DEVICE))
    return model


def detector_postprocess(results: Instances, output_height: int, output_width: int):
    """wsovod/modeling/postprocessing.py:8-82 (boxes only): rescale to the requested output size."""
    scale_x, scale_y = output_width / results.image_size[1], output_height / results.image_size[0]
    out = Instances((output_height, output_width), **results.get_fields())
    boxes = out.pred_boxes.clone()
    boxes.scale(scale_x, scale_y)
    boxes.clip(out.image_size)
    out.pred_boxes = boxes
    return out[boxes.nonempty()]


@META_ARCH_REGISTRY.register()
class GeneralizedRCNN_WSOVOD(nn.Module):
    @configurable
    def __init__(self, *, cfg=None, backbone, data_aware_head=None, proposal_generator, roi_heads,
                 pixel_mean: Tuple[float], pixel_std: Tuple[float], input_format: Optional[str] = None,
                 vis_period: int = 0):
        super().__init__()
        self.cfg = cfg
        self.backbone = backbone
        self.data_aware_head = data_aware_head
        self.proposal_generator = proposal_generator
        self.roi_heads = roi_heads
        self.input_format = input_format
        self.vis_period = 0
        self.register_buffer("pixel_mean", torch.tensor(pixel_mean).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.tensor(pixel_std).view(-1, 1, 1), False)
        self._mean, self._std = [float(v) for v in pixel_mean], [float(v) for v in pixel_std]
        self.logger = logging.getLogger(__name__)
        self.classifier = None
        # MODEL.HIP.PRECISION (layers/precision.py:TABLE): the modules see the record's forward name, the entry points enter
        # its x3 mode, f16mx selection and backward split (_entered).  Without a cfg: as the backbone's precision string says
        self.hip_precision = P.of(cfg.MODEL.HIP.PRECISION if cfg is not None else getattr(backbone, "precision", "bf16"))
        # MODEL.HIP.MX_RANGE_GUARD: None = "off" (no audit is ever launched); refused for a precision without f16mx operands
        self.mx_guard = mx_guard.from_config(cfg) if cfg is not None else None
        if self.mx_guard is not None:
            self.mx_guard.names.update({id(m): n for n, m in self.named_modules() if n})
            guard = self.mx_guard
            self.register_load_state_dict_post_hook(lambda *_a, **_k: guard.rearm())  # (holds the guard, not the model)

    @classmethod
    def from_config(cls, cfg):
        backbone = build_backbone(cfg)
        stacked, branches = getattr(backbone, "mrrp_stacked", False), getattr(backbone, "mrrp_num_branch", 1)
        if cfg.MODEL.MRRP.MRRP_ON and not stacked:
            raise NotImplementedError(f"MODEL.MRRP.MRRP_ON with {cfg.MODEL.BACKBONE.NAME}: the heads expect an MRRP backbone's "
                                      "branch-major map (built: build_mrrp_vgg_backbone with plain5 in MRRP_STAGE, "
                                      "build_mrrp_wsl_resnet_backbone with MRRP_STAGE res5)")
        if not cfg.MODEL.MRRP.MRRP_ON and stacked:
            raise NotImplementedError(f"{cfg.MODEL.BACKBONE.NAME} stacks {branches} MRRP branches along N but MODEL.MRRP.MRRP_ON is "
                                      "False: the heads would pool every box from branch 0")
        return {
            "cfg": cfg, "backbone": backbone,
            "data_aware_head": DataAwareFeaturesHead(cfg, backbone.output_shape())
            if cfg.MODEL.ROI_BOX_HEAD.OPEN_VOCABULARY.DATA_AWARE else None,
            "proposal_generator": build_proposal_generator(cfg, backbone.output_shape()), "roi_heads": build_roi_heads(cfg, backbone.output_shape()),
            "input_format": cfg.INPUT.FORMAT, "vis_period": cfg.VIS_PERIOD,
            "pixel_mean": cfg.MODEL.PIXEL_MEAN, "pixel_std": cfg.MODEL.PIXEL_STD,
        }

    @property
    def device(self):
        return self.pixel_mean.device

    # ---- input staging (H2D + padding are plumbing; normalisation is fused into the stem) ----
    def _canvas(self, batched_inputs):
        images = [x["image"] for x in batched_inputs]
        sizes = [(int(im.shape[-2]), int(im.shape[-1])) for im in images]
        Hp, Wp = max(s[0] for s in sizes), max(s[1] for s in sizes)
        canvas = self._padded_views(images, sizes, Hp, Wp, self.device)
        if canvas is not None:
            pass  # the device input stage's batch (data/train_input.py): already one zero-padded canvas, no pass at all
        elif all(im.device == self.device for im in images) and all(s == sizes[0] for s in sizes):
            canvas = self._adjacent(images)  # already resident as consecutive slices of one batch tensor: no pass at all
            if canvas is None:
                canvas = torch.stack(images)  # already resident: one gather pass
        elif all(s == sizes[0] for s in sizes):
            # host images (the DatasetMapper's format): each one is copied straight into its slot of the batch tensor --
            # no per-image device temporary and no second (stack) pass over the batch
            canvas = torch.empty((len(images), 3, Hp, Wp), dtype=images[0].dtype, device=self.device)
            for i, im in enumerate(images):
                canvas[i].copy_(im, non_blocking=True)
        else:
            canvas = torch.zeros((len(images), 3, Hp, Wp), dtype=torch.uint8, device=self.device)
            for i, im in enumerate(images):
                canvas[i, :, : sizes[i][0], : sizes[i][1]].copy_(im, non_blocking=True)
        if canvas.dtype != torch.uint8:
            raise RuntimeError("GeneralizedRCNN_WSOVOD expects uint8 CHW images (DatasetMapper format)")
        sizes_t = H.const_tensor([v for s in sizes for v in s], torch.int32, self.device).view(-1, 2)
        return canvas.contiguous(), sizes_t, sizes

    @staticmethod
    def _adjacent(images):
        """The (N,3,H,W) view over `images` when they are contiguous, equally shaped slices i = 0..N-1 of one allocation
        (a collated batch handed over as per-image views, the reference's list-of-dicts format), else None."""
        im0 = images[0]
        n = im0.numel()
        if not im0.is_contiguous() or n == 0:
            return None
        base, esz, st = im0.data_ptr(), im0.element_size(), im0.untyped_storage()
        for i, im in enumerate(images):
            if im.shape != im0.shape or not im.is_contiguous() or im.dtype != im0.dtype \
                    or im.data_ptr() != base + i * n * esz or im.untyped_storage().data_ptr() != st.data_ptr():
                return None
        if im0.storage_offset() + len(images) * n > st.nbytes() // esz:
            return None
        return im0.as_strided((len(images),) + tuple(im0.shape), (n,) + tuple(im0.stride()), im0.storage_offset())

    @staticmethod
    def _padded_views(images, sizes, Hp, Wp, device):
        """The (N,3,Hp,Wp) canvas itself when `images` are the views canvas[i, :, :h_i, :w_i], i = 0..N-1, of ONE contiguous
        uint8 canvas on `device` whose (Hp, Wp) are the batch maxima and whose producer marked it `zero_padded` (every byte
        outside the views is 0: wsovod_resample_u8_batch writes whole slots), else None.  Checked by storage and strides."""
        canvas = getattr(images[0], "_base", None)
        if canvas is None or not getattr(canvas, "zero_padded", False) or canvas.device != device \
                or canvas.dtype != torch.uint8 or tuple(canvas.shape) != (len(images), 3, Hp, Wp) or not canvas.is_contiguous():
            return None
        base, st, slot = canvas.data_ptr(), canvas.untyped_storage().data_ptr(), 3 * Hp * Wp
        for i, (im, (h, w)) in enumerate(zip(images, sizes)):
            if im.dtype != torch.uint8 or tuple(im.shape) != (3, h, w) or tuple(im.stride()) != (Hp * Wp, Wp, 1) \
                    or im.data_ptr() != base + i * slot or im.untyped_storage().data_ptr() != st:
                return None
        return canvas

    def preprocess_image(self, batched_inputs):
        """rcnn_wsovod.py:321-328: normalise, pad and batch -> ImageList (fp32 NCHW)."""
        canvas, sizes_t, sizes = self._canvas(batched_inputs)
        return ImageList(H.preprocess_image(canvas, sizes_t, self._mean, self._std), sizes)

    def _proposals(self, batched_inputs):
        assert "proposals" in batched_inputs[0]
        proposals = [x["proposals"].to(self.device) for x in batched_inputs]
        if self.proposal_generator is None:  # rcnn_wsovod.py:198-203; with an RPN the loaded boxes stay as they are
            level_ids = torch.zeros((sum(len(p) for p in proposals),), dtype=torch.int64, device=self.device)
            for p, ids in zip(proposals, level_ids.split([len(p) for p in proposals])):  # one fill, per-image views
                p.level_ids = ids
        return proposals

    def _rpn_proposals(self, images, features, batched_inputs, loaded, gt_instances=None):
        """rcnn_wsovod.py:177-197 / :267-283: RPN boxes (objectness = sigmoid, ramped by iter / MAX_ITER in
        training) followed by the loaded SAM boxes of the image."""
        proposals, _ = self.proposal_generator(images, features, gt_instances)
        ramp = self.roi_heads.iter / self.cfg.SOLVER.MAX_ITER if self.training else 1.0
        for p in proposals:
            p.objectness_logits = torch.sigmoid(p.objectness_logits) * ramp
        self.rpn_proposals = proposals
        if loaded is not None:
            for p1, p2 in zip(proposals, loaded):  # rcnn_wsovod.py:188-195 / :274-281 (the MRRP RPN tags its boxes)
                if p1.has("level_ids"):
                    p2.level_ids = self._loaded_level_ids(p1.level_ids, len(p2))
            proposals = [Instances.cat([p1, p2]) for p1, p2 in zip(proposals, loaded)]
        return proposals

    def _loaded_level_ids(self, rpn_ids, num_loaded):
        """Level ids of an image's loaded boxes: uniform integers in [min(rpn_ids), max(rpn_ids) + 1), the reference's
        torch.randint(low_id, high_id, ...) with the bounds left on the device (tensor bounds there cost a host read).
        An image without RPN boxes has no bounds to draw between: its loaded boxes get id 0 (branch 0), where the
        reference's torch.min of an empty tensor raises."""
        if len(rpn_ids) == 0:  # (a host-known length: the proposal stage's one read)
            return torch.zeros((num_loaded,), dtype=torch.int64, device=rpn_ids.device)
        low = rpn_ids.min()
        span = rpn_ids.max() + 1 - low
        return low + torch.minimum((self._level_id_draw(num_loaded, rpn_ids.device) * span).to(torch.int64), span - 1)

    def _level_id_draw(self, num_loaded, device):
        """Uniform [0, 1) numbers behind the loaded boxes' level ids.  Tests replace this to fix the draw."""
        return torch.rand((num_loaded,), dtype=torch.float64, device=device)

    _step_meta = None  # set while a whole-step HIP graph is captured: the image-level labels are static input buffers

    def _image_level_gt(self, batched_inputs):
        """get_image_level_gt (roi_heads.py:158-174) on the host copies: no device sync."""
        if self._step_meta is not None:
            return self._step_meta.image_level_gt()
        K = self.roi_heads.num_classes
        cls_list, oh = [], torch.zeros((len(batched_inputs), K), dtype=torch.float32)
        for i, x in enumerate(batched_inputs):
            gc = x["instances"].gt_classes
            if gc.is_cuda:
                return None
            u = torch.unique(gc, sorted=True).to(torch.int64)
            cls_list.append(u)
            oh[i, u] = 1.0
        cat = H.h2d_small(torch.cat(cls_list), self.device)
        off = segment_offsets([len(u) for u in cls_list], self.device)
        return cat, off, H.h2d_small(oh, self.device), max([len(u) for u in cls_list], default=0)

    def forward(self, batched_inputs, classifier=None):
        if not self.training:
            return self.inference(batched_inputs, classifier=classifier)
        return self.forward_trainable(self.forward_frozen(batched_inputs))

    # the record's fields under the names the trainer, the tools and the tests read
    x3 = property(lambda self: self.hip_precision.x3)
    mx = property(lambda self: self.hip_precision.mx)
    backward_split = property(lambda self: self.hip_precision.bwd_split)

    @property
    def mx_on(self):
        """The f16mx kernels are selected: the precision asks for them and the range guard has not fallen back to bf16x2."""
        g = getattr(self, "mx_guard", None)
        return bool(getattr(self, "mx", False)) and not (g is not None and g.fallen_back)

    @contextlib.contextmanager
    def _entered(self, *, mx=None, bwd_split=False, guard=True):
        """Context of a model entry point: the precision's state on the calling thread (mx: the f16mx kernels, mx_on unless
        given; bwd_split: the record's, the trainable part only) and, with guard, this model's range guard as its active one."""
        with P.scope(self.hip_precision, mx=self.mx_on if mx is None else mx, bwd_split=bwd_split and self.backward_split), \
                (mx_guard.active(getattr(self, "mx_guard", None)) if guard else contextlib.nullcontext()):
            yield

    def mx_guard_end_step(self, updated=True):
        """End of an ARMED training step: audit the f16mx operands of the trained weights (after the step's update, the bytes
        the optimizer kernels refreshed), poll, and act by the mode -> "ok" / "warn" / "fallback" (the caller drops what it
        captured of the f16mx kernels).  updated: the step applied an optimizer update (False: it only accumulated gradients;
        a non-finite hi then follows the mode like a saturated one)."""
        g = self.mx_guard
        if g is None or not g.armed():
            return "ok"
        for name, p in self.named_parameters():
            op = operand_cache.one_scale_mx(p) if p.requires_grad else None
            if op is not None:
                g.audit("weight:" + name, op[0], operand=True)
        return g.settle(g.poll(), updated=updated, training=True)

    @torch.no_grad()
    def forward_frozen(self, batched_inputs):
        with self._entered():
            return self._forward_frozen(batched_inputs)

    def forward_trainable(self, st):
        if self.backward_split and getattr(self, "mx", False) and getattr(self.backbone, "has_trainable_stage", False):
            raise NotImplementedError(
                'MODEL.HIP.PRECISION "parity_mx_train" needs a frozen backbone (MODEL.BACKBONE.FREEZE_AT = 5, as in every '
                "shipped WSR config): its split input gradients stop at the pooled tensor, and a trainable stage would "
                'continue them through convolution backwards that keep no hi/lo split -- use "parity_train" or "parity_mx"')
        with self._entered(bwd_split=True):
            return self._forward_trainable(st)

    @torch.no_grad()
    def inference(self, batched_inputs, detected_instances=None, do_postprocess=True, classifier=None):
        pre = getattr(self, "_pre_inference", None)  # an overlapped trainer applies its pending update first (eval / TTA
        if pre is not None:                          # hooks between steps must see the weights after optimizer.step())
            pre()
        g = getattr(self, "mx_guard", None)
        if g is None or not self.mx_on:
            with self._entered(guard=False):
                return self._inference(batched_inputs, detected_instances, do_postprocess, classifier)
        # MODEL.HIP.MX_RANGE_GUARD: every inference call is audited; the table is read after the eval tail's own host read
        # (the detections' counts), so the poll waits for nothing
        g.arm()
        g.reset()
        counter = self.roi_heads.iter_test
        try:
            with self._entered(mx=True):
                out = self._inference(batched_inputs, detected_instances, do_postprocess, classifier)
            verdict = g.settle(g.poll())
        finally:
            g.arm(False)
        if verdict != "fallback":
            return out
        # THIS batch again on the bf16x2 kernels ("parity": bf16 has fp32's exponent range); sticky -- mx_on is False from now on
        self.roi_heads.iter_test = counter
        with self._entered(mx=False, guard=False):
            return self._inference(batched_inputs, detected_instances, do_postprocess, classifier)

    def _forward_frozen(self, batched_inputs):
        """Everything of the training forward that touches NO trainable parameter: input staging, the
        frozen backbone, GAP for the data-aware head, RoI pooling with the objectness scale.  Because it
        does not depend on the weights being updated, a data-parallel trainer may run it while the previous
        step's gradient all-reduce is still in flight (wsovod_amd/engine/trainer.py)."""
        canvas, sizes_t, sizes = self._canvas(batched_inputs)
        st = {"canvas": canvas, "sizes": sizes, "gt_instances": None, "image_level_gt": None}
        self._select_source(batched_inputs, st)
        if "instances" in batched_inputs[0]:
            st["image_level_gt"] = self._image_level_gt(batched_inputs)
            # With the image-level labels already extracted on the host, the heads never read the dataset
            # boxes (weak supervision), so the instances are not copied to the device (a pageable H2D copy
            # would block the host until the stream drains).
            st["gt_instances"] = [x["instances"] if st["image_level_gt"] is not None else x["instances"].to(self.device)
                                  for x in batched_inputs]
        st["proposals"] = self._proposals(batched_inputs) if "proposals" in batched_inputs[0] else None
        if getattr(self.backbone, "has_trainable_stage", False):
            # MODEL.BACKBONE.FREEZE_AT < 5: the backbone reads weights the optimizer updates and takes part in autograd --
            # it runs in the trainable part (behind the pending update of an overlapped trainer), with gradients enabled
            st["sizes_t"] = sizes_t
            st["features"] = st["gaps"] = st["pooled"] = None
            return st
        # (a step the range guard audits keeps the eager launches: a replayed backbone graph holds no audit)
        features = self.backbone.forward_uint8(canvas, sizes_t, self._mean, self._std, allow_graph=not mx_guard.launching())
        st["features"] = features
        pool_here = self.proposal_generator is None  # with an RPN the box set depends on trainable weights: pooling moves
        fuse = contextlib.nullcontext()               # to the trainable part
        if pool_here and self.data_aware_head is not None and getattr(self.roi_heads, "pooler_type", "") == "ROIPool" \
                and st["proposals"] is not None:
            # the GAP of the data-aware head and the RoIPool pre-pass read the same res5 map: one pass (layers/hip_ops.py)
            res = self.roi_heads.box_pooler.output_size
            fuse = H.gap_with_pool_prepass(sum(len(p) for p in st["proposals"]), (res, res) if isinstance(res, int) else res)
        with fuse:
            st["gaps"] = self.data_aware_head.pooled_stats(features) if self.data_aware_head is not None else None
            st["pooled"] = self.roi_heads.pool_features(features, st["proposals"]) if pool_here else None
        return st

    def _heads_kwargs(self, st):
        return {}

    def _select_source(self, batched_inputs, st):
        pass

    def _forward_trainable(self, st):
        """The trainable remainder: data-aware MLP, neck, object mining, refinement, losses."""
        self.roi_heads.image_level_gt = st["image_level_gt"]
        if st["features"] is None:  # a trainable backbone stage: see _forward_frozen
            st["features"] = self.backbone.forward_uint8(st["canvas"], st["sizes_t"], self._mean, self._std)
            st["gaps"] = self.data_aware_head.pooled_stats(st["features"]) if self.data_aware_head is not None else None
            if self.proposal_generator is None:
                st["pooled"] = self.roi_heads.pool_features(st["features"], st["proposals"])
        daf = self.data_aware_head.from_stats(st["gaps"]) if self.data_aware_head is not None else None
        images = ImageList(st["canvas"], st["sizes"])
        proposals = st["proposals"]
        if self.proposal_generator is not None:
            proposals = self._rpn_proposals(images, st["features"], None, st["proposals"], st["gt_instances"])
        _, detector_losses = self.roi_heads(images, st["features"], proposals, daf, st["gt_instances"],
                                            append_background=True, loaded_proposals=st["proposals"],
                                            pooled=st["pooled"], **self._heads_kwargs(st))
        losses = {}
        losses.update(detector_losses)
        if self.proposal_generator is not None:  # rcnn_wsovod.py:222-223: trained from the heads' pseudo GT
            losses.update(self.proposal_generator.get_losses(self.roi_heads.proposal_targets))
        return losses

    def _inference(self, batched_inputs, detected_instances=None, do_postprocess=True, classifier=None):
        assert not self.training
        assert detected_instances is None, "forward_with_given_boxes is not on the hot path"
        canvas, sizes_t, sizes = self._canvas(batched_inputs)
        features = self.backbone.forward_uint8(canvas, sizes_t, self._mean, self._std)
        proposals = self._proposals(batched_inputs) if "proposals" in batched_inputs[0] else None
        if self.proposal_generator is not None:
            proposals = self._rpn_proposals(ImageList(canvas, sizes), features, batched_inputs, proposals)
        daf = self.data_aware_head.forward_per_image(features) if self.data_aware_head is not None else None
        if classifier is not None:
            self.classifier = classifier
        elif self.classifier is None:
            weight_path = self.cfg.MODEL.ROI_BOX_HEAD.OPEN_VOCABULARY.WEIGHT_PATH_TEST
            self.classifier = torch.as_tensor(np.load(weight_path, encoding="bytes", allow_pickle=True)).to(
                torch.float32).contiguous().to(self.device)
        results, _, all_scores, all_boxes = self.roi_heads(ImageList(canvas, sizes), features, proposals, daf, None,
                                                           self.classifier, append_background=True)
        if do_postprocess:
            return GeneralizedRCNN_WSOVOD._postprocess(results, batched_inputs, sizes)
        return results, all_scores, all_boxes

    @staticmethod
    def _postprocess(instances, batched_inputs, image_sizes):
        packed = getattr(instances, "packed", None)
        if packed is not None and len(instances):
            return GeneralizedRCNN_WSOVOD._postprocess_packed(instances, packed, batched_inputs, image_sizes)
        processed_results = []
        for results_per_image, input_per_image, image_size in zip(instances, batched_inputs, image_sizes):
            height = input_per_image.get("height", image_size[0])
            width = input_per_image.get("width", image_size[1])
            processed_results.append({"instances": detector_postprocess(results_per_image, height, width)})
        return processed_results


def _postprocess_packed(instances, packed, batched_inputs, image_sizes):
    """detector_postprocess (postprocessing.py:8-82, boxes only) for every image of the batch in one pass over the packed
    detections of the batched tail: rescale to the requested output size, clip, drop empty boxes (order kept) -- the
    same arithmetic per box as the per-image form, one host read (the surviving counts) instead of two per image."""
    det_box, det_sc, det_cls, det_prop, counts = packed
    N, k = det_sc.shape
    dev = det_box.device
    out_hw = [(int(inp.get("height", sz[0])), int(inp.get("width", sz[1]))) for inp, sz in zip(batched_inputs, image_sizes)]
    scale = H.const_tensor([v for (oh, ow), r in zip(out_hw, instances)
                            for v in (ow / r.image_size[1], oh / r.image_size[0]) * 2], torch.float32, dev).view(N, 1, 4)
    lim = H.const_tensor([float(v) for oh, ow in out_hw for v in (ow, oh, ow, oh)], torch.float32, dev).view(N, 1, 4)
    bx = torch.minimum((det_box * scale).clamp(min=0), lim)
    live = torch.arange(k, device=dev)[None] < H.const_tensor(counts, torch.int64, dev)[:, None]
    keep = live & ((bx[..., 2] - bx[..., 0]) > 0) & ((bx[..., 3] - bx[..., 1]) > 0)
    perm = torch.sort((~keep).to(torch.uint8), dim=1, stable=True).indices  # kept detections first, order preserved
    n_keep = keep.sum(dim=1).tolist()
    bx = bx.gather(1, perm[..., None].expand(N, k, 4))
    sc, cl, pi = det_sc.gather(1, perm), det_cls.gather(1, perm), det_prop.gather(1, perm)
    out = []
    for i, n in enumerate(n_keep):
        r = Instances(out_hw[i])
        r.pred_boxes = Boxes(bx[i, :n])
        r.scores, r.pred_classes, r.pred_inds = sc[i, :n], cl[i, :n], pi[i, :n]
        out.append({"instances": r})
    return out


GeneralizedRCNN_WSOVOD._postprocess_packed = staticmethod(_postprocess_packed)


@META_ARCH_REGISTRY.register()
class GeneralizedRCNN_WSOVOD_MixedDatasets(GeneralizedRCNN_WSOVOD):
    """meta_arch/rcnn_wsovod_mixed_datasets.py:28-367: a batch comes from ONE dataset (`dataset_id`); its class
    count selects the object miner and its CLIP text embeddings are handed to the refinement head per call."""

    @configurable
    def __init__(self, *, classifier_train=(), classifier_test=None, **kwargs):
        super().__init__(**kwargs)
        self.classifier_train = list(classifier_train)
        self.classifier = classifier_test

    @property
    def classifier_test(self):  # the reference's attribute name (rcnn_wsovod_mixed_datasets.py:81,319-331)
        return self.classifier

    @classmethod
    def from_config(cls, cfg):
        ret = super().from_config(cfg)

        def load(path):
            return torch.as_tensor(np.load(path, encoding="bytes", allow_pickle=True)).to(torch.float32).contiguous().to(
                cfg.MODEL.DEVICE)

        ret["classifier_train"] = [load(p) for p in cfg.DATASETS.MIXED_DATASETS.WEIGHT_PATH_TRAINS]
        ret["classifier_test"] = load(cfg.MODEL.ROI_BOX_HEAD.OPEN_VOCABULARY.WEIGHT_PATH_TEST)
        return ret

    def _select_source(self, batched_inputs, st):
        st["source_id"] = int(batched_inputs[0].get("dataset_id", 0))
        if self.training:
            self.roi_heads.select_source(st["source_id"])

    def _heads_kwargs(self, st):
        return {"classifier": self.classifier_train[st["source_id"]], "source_id": st["source_id"]}
