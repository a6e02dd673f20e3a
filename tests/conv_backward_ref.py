"""The fp64 restatement of the conv backward of a trainable stage (wsovod_amd/modeling/conv_backward.py: `_conv_dgrad`,
`_conv_wgrad`, `_block_backward`, `_stage_backward_hip`), shared by tests/test_conv_backward_ref.py (CPU) and
tests/test_gpu_conv_backward.py.  Torch on the CPU in float64; the HIP library is never touched.

The reference is LINEAR: ReLU masks and pool winners are read off the maps the caller passes (the HIP forward's own
saved maps, decoded to fp64), so no element has to be excused for a flipped mask.  Everything here is logical NCHW.

operand   "as_read": the operands are what the kernels read -- the folded weight `conv.folded(torch.float32)` (the fp32
          fold the module itself makes) rounded to the compute dtype `cd`, the FrozenBN scale as the module computes it,
          and of a bf16x2 input the hi halves (`x2=True`) for the weight gradient.  The GRADIENT is never rounded: its
          rounding to `cd` is the kernels' error, counted in `c`.
          "exact": nothing is rounded (fp64 fold of the fp32 parameters and statistics).
absolute  the same sums over |dy|, |w|, |x|, |scale| with the same 0/1 masks and pool winners: the bound map B, the sum of
          the magnitudes of all terms of each output element.
defect    (name, conv index | "shortcut" | None): one deliberate bug, for the sensitivity tests (DEFECTS below).

Tolerances: |got - ref_as_read| <= c * u * B, u = U[cd].  The c_* functions below count c from the code of conv_backward.py.
"""
import torch
import torch.nn.functional as F

U = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -9}  # the unit of the tolerances, per compute dtype
# What ONE rounding to cd costs in units of u.  bf16 keeps 8 significant bits: neighbours are 2^-7 apart, a rounding moves a
# value by up to half of that, 2^-8 = 2 u -- the u of the bf16 tolerances is HALF the format's unit roundoff, so a rounding
# counts twice.  (The first GPU run showed it: the tail conv's dW, one rounding of the gradient behind it, reached 1.9 u B.)
# fp32: 2^-24 is the unit roundoff.
ROUND = {torch.float32: 1.0, torch.bfloat16: 2.0}
WGRAD_BLOCK = 64  # the row block of the blocked weight-gradient runs (and of the two row-block defects)

DEFECTS = ("dgrad_unrotated", "w1x1_untransposed", "wgrad_no_scale", "dgrad_no_scale", "wgrad_dilation_1", "drop_last_row_block",
           "first_row_block_overwritten", "mask_from_output", "no_shortcut_dx", "pool_last_maximum")


# ---- c: counted from conv_backward.py ---------------------------------------------------------------------------------
# One fp32 accumulation of K terms (MFMA, any order, any split) errs by at most gamma_K ~ K * 2^-24 of the sum of the
# terms' magnitudes; the issue's rule doubles it: 2 * K * 2^-24, in units of u.  One extra fp32 operation is 2^-24 / u.
def acc(K, cd):
    return 2.0 * K * 2.0 ** -24 / U[cd]


def one_fp32(cd):
    return 2.0 ** -24 / U[cd]


def c_dgrad(conv, cd):
    """`_conv_dgrad` on the operands it reads: one accumulation of K = kh * kw * Cout products into fp32."""
    return acc(conv.kernel_size ** 2 * conv.out_channels, cd)


def c_wgrad(P, cd):
    """`_conv_wgrad` on the operands it reads: one accumulation over the P patch rows (the row blocks accumulate into the
    same fp32 matrix: still P terms) + the fp32 multiply `dw * scale`."""
    return acc(P, cd) + one_fp32(cd)


def block_convs(block):
    return [block.conv1, block.conv2] + ([block.conv3] if hasattr(block, "conv3") else [])


def c_block(block, P, cd):
    """-> {"dx": c, conv module: c}.  Roundings to cd on the path, ROUND[cd] units each: the gradient leaving `_masked`, once
    per conv it then enters (the weight `.to(cd)` is an operand as read: the reference holds the same rounded number, no error;
    the issue's "two roundings per conv" at u = 2^-9 and this one rounding of 2^-8 are the same 2 u); the pool backward routes
    fp32 values (none); + the longest fp32 accumulation on the path (dgrad: kh * kw * Cout, wgrad: P) + the single fp32
    operations: the add of the shortcut / identity term into dx, `dw * scale`.
      dx            n roundings (n = 2 / 3 convs: the main path; the shortcut's path has 1)           bf16: 2 n
      dW of conv i  n - i roundings: the gradient enters the n - 1 - i convs behind it, then this one  bf16: 2 (n - i)
      dW shortcut   1 rounding                                                                        bf16: 2"""
    convs = block_convs(block)
    n = len(convs)
    kd = [c.kernel_size ** 2 * c.out_channels for c in convs]
    sc = block.shortcut
    out = {"dx": ROUND[cd] * n + acc(max(kd + ([sc.out_channels] if sc is not None else [])), cd) + one_fp32(cd)}
    for i, conv in enumerate(convs):
        out[conv] = ROUND[cd] * (n - i) + acc(max([P] + kd[i + 1:]), cd) + one_fp32(cd)
    if sc is not None:
        out[sc] = ROUND[cd] + acc(P, cd) + one_fp32(cd)
    return out


def c_stage(blocks, Ps, cd):
    """A block's outputs take the error of the gradient that enters it -- the dx of every later block, carried through
    linearly (B carries it the same way) -- on top of their own: c adds up along the chain."""
    out, behind = {}, 0.0
    for block, P in zip(reversed(blocks), reversed(Ps)):
        cb = c_block(block, P, cd)
        for k, v in cb.items():
            if k != "dx":
                out[k] = v + behind
        behind += cb["dx"]
    out["dx"] = behind
    return out


# ---- operands ---------------------------------------------------------------------------------------------------------
def nchw64(t):
    """NHWC map (any device, bf16 / fp32 VALUES -- a carrier is decoded by the caller first) -> NCHW fp64 on the CPU."""
    return t.detach().to("cpu", torch.float64).permute(0, 3, 1, 2).contiguous()


def bn_scale(conv, cd=None):
    """(Cout) fp64: cd None -> the fp64 value; else the fp32 number the module computes on its own device."""
    if conv.norm is None:
        return torch.ones(conv.out_channels, dtype=torch.float64)
    n = conv.norm
    if cd is None:
        return (n.weight.detach().double() * (n.running_var.detach().double() + n.eps).rsqrt()).cpu()
    return n.scale_shift()[0].detach().double().cpu()


def folded_weight(conv, cd=None):
    """(Cout, Cin, kh, kw) fp64 of w * bn_scale: cd None -> the fp64 product; else the module's fp32 fold rounded to cd."""
    if cd is None:
        return conv.weight.detach().double().cpu() * bn_scale(conv).view(-1, 1, 1, 1)
    k = conv.kernel_size
    w = conv.folded(torch.float32)[0].to(cd).double().cpu()
    return w.view(conv.out_channels, k, k, conv.in_channels).permute(0, 3, 1, 2).contiguous()


def _is(defect, name, which=None):
    return defect is not None and defect[0] == name and (defect[1] is None or defect[1] == which)


def ref_dgrad(g, conv, cd=None, absolute=False, defect=None, which=None):
    """dL/d(input) (N, Cin, H, W) of the stride-1 same-size conv for g = dL/d(conv output) (N, Cout, H, W)."""
    w = folded_weight(conv, cd)
    if _is(defect, "dgrad_no_scale", which):
        w = conv.weight.detach().float().to(cd or torch.float64).double().cpu()
    if _is(defect, "dgrad_unrotated", which) and conv.kernel_size > 1:
        w = w.flip(2, 3)
    if _is(defect, "w1x1_untransposed", which) and conv.kernel_size == 1 and conv.in_channels == conv.out_channels:
        w = w.transpose(0, 1).contiguous()
    if absolute:
        g, w = g.abs(), w.abs()
    return F.conv_transpose2d(g, w, padding=conv.padding, dilation=conv.dilation)


def ref_wgrad(g, xin, conv, cd=None, x2=False, xhi=None, absolute=False, defect=None, which=None):
    """dL/dw (Cout, Cin, kh, kw): the correlation of g with xin at the conv's padding and dilation, times bn_scale.
    x2 (with cd): xin is the decoded value of a bf16x2 map, of which the kernel reads the hi half: `xhi` when the caller
    took the hi halves out of the carrier itself, else the bf16 rounding of the decoded value."""
    k, p, d = conv.kernel_size, conv.padding, conv.dilation
    if _is(defect, "wgrad_dilation_1", which) and d != 1:
        p, d = (k - 1) // 2, 1
    if x2 and cd is not None:
        xin = xhi if xhi is not None else xin.float().to(torch.bfloat16).double()
    N, Co, Hh, Ww = g.shape
    g2 = g.permute(0, 2, 3, 1).reshape(N * Hh * Ww, Co)  # rows in the kernels' order: (image, y, x)
    cols = F.unfold(xin, k, dilation=d, padding=p).permute(0, 2, 1).reshape(N * Hh * Ww, -1)  # columns (ci, kh, kw)
    if k > 1 and _is(defect, "drop_last_row_block", which):
        g2 = g2.clone()
        g2[(g2.size(0) - 1) // WGRAD_BLOCK * WGRAD_BLOCK:] = 0
    if k > 1 and _is(defect, "first_row_block_overwritten", which):
        g2 = g2.clone()
        g2[:WGRAD_BLOCK] = 0
    scale = bn_scale(conv, cd)
    if _is(defect, "wgrad_no_scale", which):
        scale = torch.ones_like(scale)
    if absolute:
        g2, cols, scale = g2.abs(), cols.abs(), scale.abs()
    return (g2.t() @ cols).view(Co, conv.in_channels, k, k) * scale.view(-1, 1, 1, 1)


def pool_backward(x, dy, stride, last=False):
    """The gradient of MaxPool2d(2, stride) -- stride 1: after ZeroPad2d((0, 1, 0, 1)) -- through torch's own autograd (the
    first maximum of a window in scan order takes it); last=True: the explicit sum with the LAST maximum instead."""
    xp = F.pad(x, (0, 1, 0, 1)) if stride == 1 else x
    if not last:
        xp = xp.detach().clone().requires_grad_(True)
        (gx,) = torch.autograd.grad(F.max_pool2d(xp, 2, stride), xp, dy)
    else:
        gx = pool_backward_explicit(xp, dy, stride, last=True)
    return gx[:, :, :x.shape[2], :x.shape[3]].contiguous()


def pool_backward_explicit(xp, dy, stride, last=False):
    Ho, Wo = (xp.shape[2] - 2) // stride + 1, (xp.shape[3] - 2) // stride + 1
    sl = [(slice(a, a + stride * (Ho - 1) + 1, stride), slice(b, b + stride * (Wo - 1) + 1, stride))
          for a in (0, 1) for b in (0, 1)]  # the window's cells in scan order
    cand = torch.stack([xp[:, :, sa, sb] for sa, sb in sl], -1)
    rank = torch.tensor([1.0, 2.0, 3.0, 4.0] if last else [4.0, 3.0, 2.0, 1.0], dtype=xp.dtype)
    win = ((cand == cand.max(-1, keepdim=True).values) * rank).argmax(-1)
    gx = torch.zeros_like(xp)
    for j, (sa, sb) in enumerate(sl):
        gx[:, :, sa, sb] += dy * (win == j)
    return gx


def ref_block_backward(block, ins, out, dy, need_dx, operand="as_read", cd=torch.bfloat16, x2=False, ins_hi=None,
                       absolute=False, defect=None):
    """`_block_backward` in fp64.  ins: the inputs of conv1, conv2(, conv3); out: the block's output ahead of its tail pool;
    dy: dL/d(block output) (behind the pool); all NCHW fp64; ins_hi (x2): the hi halves of `ins`, as stored.
    -> (dx or None, {conv module: dL/dw})."""
    cd = cd if operand == "as_read" else None
    assert operand in ("as_read", "exact")
    kw = dict(cd=cd, absolute=absolute, defect=defect)
    convs = block_convs(block)
    grads = {}
    if absolute:
        dy = dy.abs()
    if block.has_pool:
        dy = pool_backward(out, dy, block.pool_stride, last=_is(defect, "pool_last_maximum"))
    g = dy * (out > 0)
    g_tail = g
    dx = None
    for i in range(len(convs) - 1, -1, -1):
        conv, xin = convs[i], ins[i]
        if conv.weight.requires_grad:
            grads[conv] = ref_wgrad(g, xin, conv, x2=x2, xhi=ins_hi[i] if ins_hi else None, which=i, **kw)
        if i == 0 and not need_dx:
            break
        dx = ref_dgrad(g, conv, which=i, **kw)
        if i > 0:
            src = xin
            if _is(defect, "mask_from_output", i):
                src = ins[i + 1] if i + 1 < len(convs) else out  # the map this conv WROTE (same channels required)
                assert src.shape == xin.shape
            g = dx * (src > 0)
    sc = block.shortcut
    if sc is not None:
        if sc.weight.requires_grad:
            grads[sc] = ref_wgrad(g_tail, ins[0], sc, x2=x2, xhi=ins_hi[0] if ins_hi else None, which="shortcut", **kw)
        if need_dx and not _is(defect, "no_shortcut_dx"):
            dx = dx + ref_dgrad(g_tail, sc, which="shortcut", **kw)
    elif need_dx and not _is(defect, "no_shortcut_dx"):
        dx = dx + g_tail
    return (dx if need_dx else None), grads


def ref_stage_backward(blocks, acts, dy, need_dx, **kw):
    """`_stage_backward_hip`'s chain: acts = [(ins, out) or (ins, out, ins_hi)] per block.  -> (dx or None, {conv: dL/dw})."""
    grads, g = {}, dy
    for bi in range(len(blocks) - 1, -1, -1):
        ins, out, *hi = acts[bi]
        g, gb = ref_block_backward(blocks[bi], ins, out, g, bi > 0 or need_dx, ins_hi=hi[0] if hi else None, **kw)
        grads.update(gb)
    return g, grads


# ---- the blocks under test (issue: the smallest geometries at which the paths differ) -----------------------------------
MAPS = ((2, 9, 11), (3, 7, 13))  # (N, H, W): P = 198 and 273, neither a multiple of 64; odd sizes floor the stride-2 pool


def seed_bn(module, seed):
    """Seeded non-trivial FrozenBN statistics on every conv under `module`: scales log-uniform in 0.25 .. 4, a quarter of
    them negative."""
    from wsovod_amd.modeling.backbone import FrozenBatchNorm2d

    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, FrozenBatchNorm2d):
            n = m.num_features
            var = 0.5 + 1.5 * torch.rand(n, generator=g)
            scale = torch.exp2(4 * torch.rand(n, generator=g) - 2) * torch.where(torch.rand(n, generator=g) < 0.25, -1.0, 1.0)
            with torch.no_grad():
                m.running_var.copy_(var)
                m.weight.copy_(scale * (var + m.eps).sqrt())
                m.bias.copy_(0.5 * torch.randn(n, generator=g))
                m.running_mean.copy_(0.5 * torch.randn(n, generator=g))
    return module


def make_block(kind, seed=0):
    from wsovod_amd.modeling.backbone import BasicBlock, BottleneckBlock

    torch.manual_seed(1000 + seed)
    b = {
        "basic_identity": lambda: BasicBlock(64, 64, norm="FrozenBN"),
        "basic_projection": lambda: BasicBlock(64, 128, norm="FrozenBN"),
        "basic_pool_s2": lambda: BasicBlock(64, 64, stride=2, norm="FrozenBN", has_pool=True),
        "basic_pool_s1": lambda: BasicBlock(128, 128, stride=1, norm="FrozenBN", has_pool=True),
        "bottleneck_identity": lambda: BottleneckBlock(256, 256, bottleneck_channels=64, norm="FrozenBN"),
        "bottleneck_dilated_projection": lambda: BottleneckBlock(128, 256, bottleneck_channels=64, norm="FrozenBN", dilation=2),
        # (CPU only: the one form with a 1x1 conv of Cin == Cout, where a transposed weight is no shape error)
        "bottleneck_square": lambda: BottleneckBlock(64, 64, bottleneck_channels=64, norm="FrozenBN"),
    }[kind]()
    return seed_bn(b, 2000 + seed)


BLOCK_KINDS = ("basic_identity", "basic_projection", "basic_pool_s2", "basic_pool_s1", "bottleneck_identity",
               "bottleneck_dilated_projection")
