"""Test-time augmentation with the views built and merged on the device (MODEL.HIP.TTA_DEVICE, default off).

The mappers and wrappers here extend those of `test_time_augmentation.py` (the host route: PIL bilinear on the host, one
upload per view, every view's boxes read back, mapped in numpy and uploaded again before `torch.mean` / `torch.cat`) by one
argument, `device_views`.  With it off each call goes straight to the parent class: the host route's code, untouched.  With
it on:

* the image is uploaded once; each size's view and its mirror are ONE `hip_ops.resample_u8` call (Pillow's fixed-point
  filter, byte for byte) whose two slices are adjacent, so a wrapper with batch_size=2 hands them to the backbone as a
  batch without a copy;
* AVG back-maps and averages all views in one `hip_ops.tta_avg` launch (fp64 sums, one rounding: it differs from the host
  route's float32 `torch.mean` by rounding only); UNION back-maps each view with one `hip_ops.tta_map_boxes` launch (the
  host route's bits).  Nothing is read back between the first view's forward and the merge.

Proposal forward-mapping stays on the host in both routes.  `wsovod_amd.modeling` exports the wrappers of this module.
"""
import copy

import numpy as np
import torch

from ..config import configurable
from ..data.proposals import HFlipTransform, ResizeTransform, transform_proposals
from ..layers import hip_ops as H
from ..structures import Boxes, Instances
from . import test_time_augmentation as host
from .test_time_augmentation import _InvertibleList, _resize_image, _shortest_edge_size

__all__ = ["DatasetMapperTTAAVG", "DatasetMapperTTAUNION", "GeneralizedRCNNWithTTAAVG", "GeneralizedRCNNWithTTAUNION",
           "back_params", "back_map_host"]


def back_params(tfm):
    """What `tfm.inverse().apply_box` multiplies and subtracts, for a view's list [pre-resize,] resize [, flip]:
    (flip, flip_w, sx, sy, pre) -- un-flip about flip_w, scale by the doubles (sx, sy), then by pre = (px, py) or None --
    each the expression ResizeTransform / HFlipTransform evaluate.  None for any other list (the host route maps it)."""
    ts = list(tfm.transforms)
    flip_w = ts.pop().width if ts and isinstance(ts[-1], HFlipTransform) else None
    if not 1 <= len(ts) <= 2 or not all(isinstance(t, ResizeTransform) for t in ts):
        return None
    fac = [(t.w * 1.0 / t.new_w, t.h * 1.0 / t.new_h) for t in ts]  # the inverse resize's new_w * 1.0 / w
    return (flip_w is not None, flip_w if flip_w is not None else 0, fac[-1][0], fac[-1][1], fac[0] if len(ts) == 2 else None)


def back_map_host(boxes, params):
    """The float32 arithmetic of `_InvertibleList.inverse().apply_box` on (M, 4) boxes, restated operation by operation
    from `back_params`: what wsovod_tta_map_boxes / wsovod_tta_avg compute per box (tests hold all three together)."""
    flip, flip_w, sx, sy, pre = params
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    x, y = b[:, [0, 2]], b[:, [1, 3]]
    if flip:
        x = np.float32(flip_w) - x
    x, y = x * np.float32(sx), y * np.float32(sy)
    if pre is not None:
        x, y = x * np.float32(pre[0]), y * np.float32(pre[1])
    return np.stack([x.min(axis=1), y.min(axis=1), x.max(axis=1), y.max(axis=1)], axis=1)


def _xforms(tfms):
    """One wsovod_tta_xform per view, or None when a view's list is not of the shape the kernels map."""
    params = [back_params(t) for t in tfms]
    return None if any(p is None for p in params) else [H.tta_xform(*p) for p in params]


class DatasetMapperTTAAVG(host.DatasetMapperTTAAVG):
    """device_views: False (the parent's call: PIL on the host, CPU images) | True or a device (the image uploaded once,
    every size's views from one hip_ops.resample_u8 call, device images)."""

    @configurable
    def __init__(self, min_sizes, max_size, flip, proposal_topk, device_views=False):
        host.DatasetMapperTTAAVG.__init__(self, min_sizes, max_size, flip, proposal_topk)
        self.device_views = device_views

    @classmethod
    def from_config(cls, cfg):
        return {**super().from_config(cfg), "device_views": cfg.MODEL.HIP.TTA_DEVICE}

    def __call__(self, dataset_dict):
        if not self.device_views:
            return host.DatasetMapperTTAAVG.__call__(self, dataset_dict)
        image = dataset_dict["image"]
        shape = (int(image.shape[1]), int(image.shape[2]))
        orig_shape = (dataset_dict["height"], dataset_dict["width"])
        pre = [ResizeTransform(orig_shape[0], orig_shape[1], shape[0], shape[1])] if shape != orig_shape else []
        device_image = image.to("cuda" if self.device_views is True else self.device_views)
        rest = {k: v for k, v in dataset_dict.items() if k != "image"}  # every view gets its own image below
        ret = []
        for min_size in self.min_sizes:
            nh, nw = _shortest_edge_size(shape[0], shape[1], min_size, self.max_size)
            try:
                images = H.resample_u8(device_image, nh, nw, self.flip)
            except H.Unsupported:  # a size the kernel refuses is never approximated: this size's views come from PIL
                resized = _resize_image(image.permute(1, 2, 0).cpu().numpy(), nh, nw)
                images = [torch.from_numpy(np.ascontiguousarray((resized[:, ::-1] if flip else resized).transpose(2, 0, 1)))
                          for flip in ([False, True] if self.flip else [False])]
            for new_image, flip in zip(images, [False, True]):
                tf = pre + [ResizeTransform(shape[0], shape[1], nh, nw)] + ([HFlipTransform(nw)] if flip else [])
                dic = copy.deepcopy(rest)
                dic["transforms"] = _InvertibleList(tf)
                dic["image"] = new_image
                if self.proposal_topk and "proposal_boxes" in dic:
                    transform_proposals(dic, (nh, nw), dic["transforms"], proposal_topk=self.proposal_topk)
                elif "proposals" in dic:  # already-mapped Instances: move the boxes with the view, keep their order
                    p = dic["proposals"]
                    q = Instances((nh, nw), **p.get_fields())
                    view = _InvertibleList(tf[len(pre):])  # the mapped boxes live in the input image's frame
                    boxes = Boxes(torch.from_numpy(view.apply_box(p.proposal_boxes.tensor.cpu().numpy())).float())
                    boxes.clip(q.image_size)
                    q.proposal_boxes = boxes
                    dic["proposals"] = q
                ret.append(dic)
        return ret


class DatasetMapperTTAUNION(host.DatasetMapperTTAUNION, DatasetMapperTTAAVG):
    """The parent's proposal handling around the views of the mapper above (its `super().__call__` resolves to it)."""


class _DeviceViews:
    """`device_views` (None: MODEL.HIP.TTA_DEVICE) on a TTA wrapper: back-map and merge the views' predictions on the device;
    the mapper built here builds its views there too (a mapper handed in keeps its own setting)."""

    def __init__(self, cfg, model, tta_mapper=None, batch_size=1, device_views=None):
        on = bool(cfg.MODEL.HIP.TTA_DEVICE if device_views is None else device_views)
        if tta_mapper is None:
            tta_mapper = self._mapper_cls(**{**self._mapper_cls.from_config(cfg), "device_views": model.device if on else False})
        super().__init__(cfg, model, tta_mapper, batch_size)
        self.device_views = on


class GeneralizedRCNNWithTTAAVG(_DeviceViews, host.GeneralizedRCNNWithTTAAVG):
    _mapper_cls = DatasetMapperTTAAVG

    def _get_augmented_boxes(self, augmented, tfms):
        xforms = _xforms(tfms) if self.device_views and len(tfms) <= H.TTA_MAX_VIEWS else None
        if xforms is None:
            return super()._get_augmented_boxes(augmented, tfms)
        _, all_scores, all_boxes = self._run_model(augmented)
        boxes, scores = self._average(all_boxes, all_scores, xforms)
        return boxes, scores, None

    def _average(self, all_boxes, all_scores, xforms):
        """Per view (1, R, 4C) boxes in the view's frame and (1, R, K+1) scores -> their means in the original frame."""
        assert all(b.shape[0] == 1 for b in all_boxes)
        return H.tta_avg([b[0] for b in all_boxes], [s[0] for s in all_scores], xforms)


class GeneralizedRCNNWithTTAUNION(_DeviceViews, host.GeneralizedRCNNWithTTAUNION):
    _mapper_cls = DatasetMapperTTAUNION

    def _get_augmented_boxes(self, augmented, tfms):
        xforms = _xforms(tfms) if self.device_views else None
        if xforms is None:
            return super()._get_augmented_boxes(augmented, tfms)
        outputs, _, _ = self._run_model(augmented)
        all_boxes, all_scores, all_classes = [], [], []
        for output, xform in zip(outputs, xforms):
            all_boxes.append(H.tta_map_boxes(output.pred_boxes.tensor, xform))
            all_scores.extend(output.scores)
            all_classes.extend(output.pred_classes)
        return torch.cat(all_boxes, dim=0), all_scores, all_classes
