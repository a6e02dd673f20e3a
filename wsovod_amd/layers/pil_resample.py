"""Pillow's 8-bit bilinear resample (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc,
ImagingResampleHorizontal_8bpc / Vertical_8bpc) restated in numpy: the coefficient tables `wsovod_resample_u8` reads, and a
host two-pass over them that tests hold against `PIL.Image.resize(..., BILINEAR)` byte for byte.

Per axis (n_in -> n_out), in fp64: scale = n_in / n_out, filterscale = max(scale, 1), support = 1.0 * filterscale,
ksize = int(ceil(support)) * 2 + 1; output xx has center = (xx + 0.5) * scale, first tap xmin = max(int(center - support +
0.5), 0) and xmax = min(int(center + support + 0.5), n_in) - xmin taps of weight tri((x + xmin - center + 0.5) / filterscale),
normalised by their sum taken in tap order, then scaled by 2^22 and rounded half away from zero by truncation.  A pass is
clamp((2^21 + sum pixel * k) >> 22, 0, 255) into uint8; the horizontal pass runs first, and its rounded uint8 result is what
the vertical pass reads.
"""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2

_TABLES = {}


def resample_table(n_in, n_out):
    """(kk (n_out, ksize) int32, bounds (n_out, 2) int32 = (first tap, taps), ksize) of one axis; cached per size pair."""
    key = (int(n_in), int(n_out))
    hit = _TABLES.get(key)
    if hit is not None:
        return hit
    n_in, n_out = key
    assert n_in > 0 and n_out > 0, key
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)  # astype truncates toward zero, as C's (int)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in) - xmin
    assert int(xmax.max()) <= ksize and int(xmax.min()) >= 0
    w = np.zeros((n_out, ksize), dtype=np.float64)
    ww = np.zeros(n_out, dtype=np.float64)
    for x in range(ksize):  # tap by tap, so that ww accumulates in Pillow's order
        a = np.abs((x + xmin - center + 0.5) * ss)
        wx = np.where((x < xmax) & (a < 1.0), 1.0 - a, 0.0)
        w[:, x] = wx
        ww = ww + wx
    nz = ww != 0.0
    w[nz] = w[nz] / ww[nz, None]
    v = w * (1 << PRECISION_BITS)
    kk = np.where(w < 0, -0.5 + v, 0.5 + v).astype(np.int32)
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    if len(_TABLES) > 256:
        _TABLES.clear()
    _TABLES[key] = (kk, bounds, ksize)
    return _TABLES[key]


def _pass(a, axis, n_out):
    n_in = a.shape[axis]
    kk, bounds, ksize = resample_table(n_in, n_out)
    a = np.moveaxis(a, axis, -1).astype(np.int32)
    acc = np.full(a.shape[:-1] + (n_out,), 1 << (PRECISION_BITS - 1), dtype=np.int32)
    for t in range(ksize):
        live = t < bounds[:, 1]
        acc += a[..., np.minimum(bounds[:, 0] + t, n_in - 1)] * np.where(live, kk[:, t], 0).astype(np.int32)
    return np.moveaxis(np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8), -1, axis)


def resample_u8_host(img, new_h, new_w, channels_first=False):
    """The two-pass on a uint8 (H, W, 3) image, or (3, H, W) with channels_first: what Image.resize((new_w, new_h),
    BILINEAR) returns.  An axis that keeps its size is skipped."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    ax_h, ax_w = (1, 2) if channels_first else (0, 1)
    if img.shape[ax_w] != new_w:
        img = _pass(img, ax_w, new_w)
    if img.shape[ax_h] != new_h:
        img = _pass(img, ax_h, new_h)
    return np.ascontiguousarray(img)
