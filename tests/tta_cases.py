"""Shared cases of the device test-time augmentation tests (test_tta_device_host.py, test_gpu_tta_device.py): seeded source
images, the resample targets, view transform lists and boxes."""
import numpy as np
import torch
from PIL import Image

from wsovod_amd.data.proposals import HFlipTransform, ResizeTransform

SOURCES = [(256, 352), (37, 53), (5, 7), (1, 9), (333, 500), (480, 640)]


def source_image(h, w):
    """Seeded uint8 (h, w, 3); the (37, 53) one is a random 0 / 255 pattern (every rounding and clamp at full swing)."""
    rng = np.random.default_rng(1000 * h + w)
    if (h, w) == (37, 53):
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def targets(h, w):
    """Down on both axes, (256, 352) (the identity for that source), one pass only (either), extreme down, one pixel, up on
    both axes, unequal ratios, mixed up / down."""
    return [(192, 264), (256, 352), (h, 2 * w), (2 * h + 1, w), (3, 4), (1, 1), (3 * h + 2, 3 * w + 1),
            (max(1, h // 3), max(1, w // 5)), (480, 660)]


def pil_resize(img_hwc, nh, nw):
    return np.asarray(Image.fromarray(img_hwc).resize((nw, nh), Image.BILINEAR))


def boxes_f32(n, w, h, seed):
    g = torch.Generator().manual_seed(seed)
    b = torch.rand((n, 4), generator=g) * torch.tensor([w, h, w, h]) * 1.1 - 5.0
    b[::7, [0, 2]] = b[::7, [2, 0]]  # some boxes with x0 > x1: min / max over the corners matters
    return b.numpy().astype(np.float32)


VIEW_LISTS = {
    "resize": lambda: [ResizeTransform(256, 352, 192, 264)],
    "resize_up": lambda: [ResizeTransform(256, 352, 1152, 1584)],
    "resize_flip": lambda: [ResizeTransform(256, 352, 192, 264), HFlipTransform(264)],
    "resize_up_flip": lambda: [ResizeTransform(256, 352, 1152, 1584), HFlipTransform(1584)],
    "pre_resize": lambda: [ResizeTransform(375, 500, 256, 352), ResizeTransform(256, 352, 1152, 1584)],
    "pre_resize_flip": lambda: [ResizeTransform(375, 500, 256, 352), ResizeTransform(256, 352, 192, 264), HFlipTransform(264)],
    "odd": lambda: [ResizeTransform(333, 500, 480, 721), HFlipTransform(721)],
}
