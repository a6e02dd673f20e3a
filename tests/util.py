import torch


def random_rois(R, n_img, H_img, W_img, seed=0, edge_cases=True):
    """(R,5) fp32 [batch, x0, y0, x1, y1] in image pixels, with the reference-relevant edge cases."""
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(R, generator=g) * (W_img - 17)
    y0 = torch.rand(R, generator=g) * (H_img - 17)
    w = 16 + torch.rand(R, generator=g) * (min(400, W_img) - 16)
    h = 16 + torch.rand(R, generator=g) * (min(300, H_img) - 16)
    b = torch.randint(0, n_img, (R,), generator=g).float()
    rois = torch.stack([b, x0, y0, (x0 + w).clamp(max=W_img), (y0 + h).clamp(max=H_img)], 1)
    if edge_cases and R >= 8:
        rois[0, 1:] = torch.tensor([-50.0, -50.0, -10.0, -10.0])  # fully outside (top-left)
        rois[1, 1:] = torch.tensor([W_img - 10.0, H_img - 10.0, W_img + 100.0, H_img + 100.0])  # spills out
        rois[2, 1:] = torch.tensor([100.0, 100.0, 100.0, 100.0])  # zero-size -> 1x1
        rois[3, 1:] = torch.tensor([300.0, 200.0, 100.0, 50.0])  # malformed (end < start)
        rois[4, 1:] = torch.tensor([0.0, 0.0, float(W_img), float(H_img)])  # whole image
        rois[5, 1:] = torch.tensor([4.0, 4.0, 11.9, 11.9])  # sub-cell box: empty bins
        rois[6, 1:] = torch.tensor([3.5, 3.5, 12.5, 20.5])  # .5 rounding (half away from zero)
        rois[7, 1:] = torch.tensor([W_img + 50.0, H_img + 50.0, W_img + 90.0, H_img + 90.0])  # fully outside
    return rois


# ---- input builders of tests/test_gpu_elementwise.py ---------------------------------------------------------------
SENTINEL = -7777.0  # (rounded to the buffer's dtype when it is filled; compared through the same rounding)


def bits(t):
    """Integer view of a float tensor: comparisons through it count NaN payloads and the sign of zero."""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def odd_view(shape, dtype, ld, offset, device, tail=11):
    """((rows, cols) view with row stride ld >= cols, its buffer): the view starts `offset` elements into a flat buffer
    pre-filled with SENTINEL, which forces the kernels' non-16-byte-aligned / odd-leading-dimension paths."""
    rows, cols = shape
    assert ld >= cols and rows >= 1
    buf = torch.full((offset + (rows - 1) * ld + cols + tail,), SENTINEL, dtype=dtype, device=device)
    return buf.as_strided((rows, cols), (ld, 1), offset), buf


def outside_intact(buf, view):
    """True when every element of `buf` outside `view` (an odd_view of it, or any 2-D strided view) still holds SENTINEL."""
    rows, cols = view.shape
    off = view.storage_offset() - buf.storage_offset()
    inside = torch.zeros(buf.numel(), dtype=torch.bool)
    idx = off + torch.arange(rows)[:, None] * view.stride(0) + torch.arange(cols)[None, :] * view.stride(1)
    inside[idx.reshape(-1)] = True
    rest = buf.detach().reshape(-1).cpu()[~inside]
    return bool((bits(rest) == bits(torch.full((1,), SENTINEL, dtype=buf.dtype))).all())
