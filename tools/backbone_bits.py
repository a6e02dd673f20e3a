"""The backbones' outputs as SHA-256 digests of their raw bytes, and the launches behind them per kernel: the evidence that a
change of the host code between two commits changed neither a bit nor a launch.

    WSOVOD_DETERMINISTIC=1 python tools/backbone_bits.py --out bits.json          (one MI355X)
    python tools/backbone_bits.py --compare parent_a.json parent_b.json branch.json --out comparison.json

The file uses only the surface that both commits have -- config -> `build_backbone`, `forward_uint8`, `hip_conv`,
`hip_conv_branches`, autograd -- so the identical file runs on a checkout of the other commit.  Module-level limits that tests
lower (CONV_MAX_OPERAND_BYTES, WGRAD_PATCH_BYTES) are set on every module of wsovod_amd.modeling that has the name.

Pass 1 computes the digests on eager launches; pass 2 runs the same cases again with the per-launch profile on and records
{kernel: launches} per case (weight operands are cached by then: the counts are those of a steady-state call).

Cases (a 96 x 128 canvas, image sizes below the canvas so padding rows exist):
    resnet/R{18,50}/{bf16,fp32,parity,parity_mx}/fuse{1,0}[/blocks]   2 images; blocks: CONV_MAX_OPERAND_BYTES = one image's
                                                                     largest map; n5: 5 images in blocks of two
    vgg16, vgg16_mrrp (dilations 1, 2, 3; WSOVOD_BRANCH_BATCHED 0 / 1) in the four precisions [/blocks]
    rpn_head_conv/parity                                              the 3x3 conv with a real-fp32 output, 2 x 12 x 16 x 512
    grad/R18/freeze{0,2}/{bf16,fp32,parity}[/row_blocks]              weight gradients of sum(res5 * fixed_random); the
                                                                     input-side gradients of the later convs are inside those
                                                                     of the earlier ones
    front/...                                                         hip_ops calls the backbones at this size do not reach,
                                                                     each on the shape of the test that covers it: split-K
                                                                     gemm_nt (bf16, bf16x2), the f16mx GEMM's split last
                                                                     round, gemm_tn with every tile split / a split last
                                                                     round, gemm_tn_sgd, mask_transpose with a column sum,
                                                                     weighted_ce_forward
"precision parity_mx": MX_MIN_TILES is lowered to 1 so that the crossing to the f16mx kernels happens at this size.

--compare leaves out every entry whose digest differs between the two parent runs (a result that depends on atomics by
design) and names it; none of the cases above is expected there outside stream capture.
"""
import argparse
import hashlib
import json
import os
import sys

os.environ.setdefault("WSOVOD_DETERMINISTIC", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

PRECISIONS = ("bf16", "fp32", "parity", "parity_mx")
HP, WP = 96, 128


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def set_everywhere(name, value):
    """`name` = value on every loaded module of wsovod_amd.modeling that defines it -> [(module, old value)]."""
    old = []
    for modname, m in list(sys.modules.items()):
        if modname.startswith("wsovod_amd.modeling") and m is not None and name in vars(m):
            old.append((m, getattr(m, name)))
            setattr(m, name, value)
    assert old, name
    return old


def restore(name, old):
    for m, v in old:
        setattr(m, name, v)


class Cases:
    def __init__(self, gpu):
        from wsovod_amd.layers import precision as P
        from wsovod_amd.modeling.backbone import FrozenForwardMixin

        self.gpu, self.P = gpu, P
        self.models = {}
        FrozenForwardMixin.MX_MIN_TILES = 1
        g = torch.Generator().manual_seed(1234)
        self.canvas = torch.randint(0, 256, (5, 3, HP, WP), generator=g, dtype=torch.uint8).to(gpu)
        self.sizes = torch.tensor([[HP - 5 - 8 * (i % 3), WP - 3 - 16 * (i % 2)] for i in range(5)], dtype=torch.int32, device=gpu)
        self.random = {}

    def backbone(self, kind, precision, freeze_at=None):
        from wsovod_amd.modeling.meta_arch import build_backbone
        from wsovod_amd.testing import hot_path_cfg

        key = (kind, precision, freeze_at)
        if key not in self.models:
            kw = dict(depth=int(kind[1:])) if kind.startswith("R") else dict(backbone="vgg16", mrrp=kind == "vgg16_mrrp")
            cfg = hot_path_cfg(precision=precision, device="cuda:0", freeze_at=freeze_at, **kw)
            if kind == "vgg16_mrrp":
                cfg.MODEL.MRRP.BRANCH_DILATIONS = [1, 2, 3]
            torch.manual_seed(0)
            bb = build_backbone(cfg).to(self.gpu)
            with torch.no_grad():  # (raw-scale pixels -> O(1) maps, as wsovod_amd.testing.build_hot_path_model)
                if kind.startswith("R"):
                    bb.stem.conv1.norm.weight.fill_(1.0 / 64.0)
                else:
                    bb.plain1[0].conv1.weight.mul_(1.0 / 64.0)
            mean, std = tuple(float(v) for v in cfg.MODEL.PIXEL_MEAN), tuple(float(v) for v in cfg.MODEL.PIXEL_STD)
            self.models[key] = (bb, mean, std)
        return self.models[key]

    def forward(self, kind, precision, n, freeze_at=None):
        from wsovod_amd.layers import hip_ops as H

        bb, mean, std = self.backbone(kind, precision, freeze_at)
        with H.mx_mode(self.P.of(precision).mx):
            return bb, bb.forward_uint8(self.canvas[:n].contiguous(), self.sizes[:n].contiguous(), mean, std)

    def fixed_random(self, t):
        key = tuple(t.shape)
        if key not in self.random:
            self.random[key] = torch.randn(key, generator=torch.Generator().manual_seed(99), dtype=torch.float32).to(self.gpu)
        return self.random[key]

    def all(self):
        """-> (name, thunk -> {tensor name: tensor}) in a fixed order."""
        esize = lambda precision: 2 if precision == "bf16" else 4
        one_map = lambda precision: 48 * 64 * 64 * esize(precision) + 1  # the largest per-image map behind the first conv

        def fwd(kind, precision, n, env=(), limit=None):
            def run():
                saved = {k: os.environ.get(k) for k, _ in env}
                os.environ.update(dict(env))
                old = set_everywhere("CONV_MAX_OPERAND_BYTES", limit) if limit is not None else None
                try:
                    with torch.no_grad():
                        return {k: v.permute(0, 2, 3, 1) for k, v in self.forward(kind, precision, n)[1].items()}
                finally:
                    if old is not None:
                        restore("CONV_MAX_OPERAND_BYTES", old)
                    for k, v in saved.items():
                        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            return run

        for depth in ("R18", "R50"):
            for precision in PRECISIONS:
                for fuse in ("1", "0"):
                    env = (("WSOVOD_FUSE_SHORTCUT", fuse),)
                    base = f"resnet/{depth}/{precision}/fuse{fuse}"
                    yield base, fwd(depth, precision, 2, env)
                    yield base + "/blocks", fwd(depth, precision, 2, env, one_map(precision))
                yield f"resnet/{depth}/{precision}/fuse1/n5_blocks", fwd(depth, precision, 5, (("WSOVOD_FUSE_SHORTCUT", "1"),),
                                                                        2 * one_map(precision))
        for precision in PRECISIONS:
            yield f"vgg16/{precision}", fwd("vgg16", precision, 2)
            yield f"vgg16/{precision}/blocks", fwd("vgg16", precision, 2, (), 2 * one_map(precision))  # (plain1: 96 x 128 x 64)
            for batched in ("0", "1"):
                env = (("WSOVOD_BRANCH_BATCHED", batched),)
                yield f"vgg16_mrrp/{precision}/batched{batched}", fwd("vgg16_mrrp", precision, 2, env)
                yield f"vgg16_mrrp/{precision}/batched{batched}/n5_blocks", fwd("vgg16_mrrp", precision, 5, env,
                                                                               4 * one_map(precision))
        yield "rpn_head_conv/parity", self.rpn_head_conv
        for freeze_at in (0, 2):
            for precision in ("bf16", "fp32", "parity"):
                yield f"grad/R18/freeze{freeze_at}/{precision}", self.grads(freeze_at, precision)
        yield "grad/R18/freeze0/parity/row_blocks", self.grads(0, "parity", 2048 * 9 * 64 * 4)
        yield from self.fronts()

    def fronts(self):
        """The split / workspace paths of the GEMM fronts and their two neighbours (tests/test_gpu_gemm.py, test_gpu_f16mx.py,
        test_gpu_head_kernels.py, test_gpu_fused_sgd.py name these shapes as the smallest at which each split engages)."""
        from wsovod_amd.layers import hip_ops as H

        gpu = self.gpu
        rand = lambda seed, *shape: torch.rand(shape, generator=torch.Generator().manual_seed(seed)).to(gpu) - 0.5
        randn = lambda seed, *shape: torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(gpu)

        def split_k(x2):  # 3 x 5 tiles, K = 129 K-steps
            def run():
                M, N, K = 520, 1056 if x2 else 1032, 8192 + 64
                a, b, bias = rand(1, M, K), rand(2, N, K), randn(3, N)
                if x2:
                    return {"c": H.gemm_nt(H.x2_encode(a), H.x2_encode(b), x2=True, out_dtype=torch.float32, bias=bias, relu=True)}
                kw = dict(bias=bias, relu=True, residual=randn(4, M, N).to(torch.bfloat16), alpha=0.5, dropout_p=0.5, dropout_seed=77)
                return {"c": H.gemm_nt(a.to(torch.bfloat16), b.to(torch.bfloat16), out_dtype=torch.float32, **kw)}
            return run

        def mx_tail():  # CUs + 18 row tiles: the last round's 18 tiles as K slices
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            M, N, K = (cus + 18) * 256 - 100, 256, 1536
            A, _ = H.mx_encode(torch.relu(randn(5, M, K)), unit=True)
            B, sb = H.mx_encode(randn(6, N, K) * 0.03)
            return {"c": H.gemm_mx(A, None, B, sb, bias=randn(7, N), relu=True, dropout_p=0.5, dropout_seed=11)}

        def tn(Mred, NI, NJ):
            def run():
                P, Q = rand(8, Mred, NI).to(torch.bfloat16), rand(9, Mred, NJ).to(torch.bfloat16)
                old, H.DETERMINISTIC = H.DETERMINISTIC, False  # (the deterministic mode switches the split tail off)
                try:
                    return {"dw": H.gemm_tn(P, Q), "dw_acc": H.gemm_tn(P, Q, out=randn(10, NI, NJ), alpha=0.5, accumulate=True)}
                finally:
                    H.DETERMINISTIC = old
            return run

        def tn_sgd():  # 3 x 5 ragged tiles, two steps, the second with the rate in device memory
            Mred, NI, NJ = 300, 520, 1056
            dA, x = (randn(11, Mred, NI) * 0.1).to(torch.bfloat16), H.x2_encode(randn(12, Mred, NJ))
            w, buf = randn(13, NI, NJ) * 0.05, torch.zeros(NI, NJ, device=gpu)
            shadow = H.x2_encode(w)
            H.gemm_tn_sgd(dA, x, w, buf, shadow, 0.013, 5e-4, 0.9, q_x2=True)
            H.gemm_tn_sgd(dA, x, w, buf, shadow, torch.tensor([0.013], device=gpu), 5e-4, 0.9, q_x2=True)
            return {"param": w, "momentum": buf, "shadow": shadow}

        def colsum():
            M, N = 8192, 1024
            cs = torch.zeros(N, device=gpu)
            dA, _ = H.mask_transpose(randn(14, M, N), randn(15, M, N), 0.5, torch.bfloat16, want_t=False, colsum=cs)
            return {"dA": dA, "colsum": cs}

        def ce():
            M, K = 16384, 20
            gt = torch.randint(-1, K + 1, (M,), generator=torch.Generator().manual_seed(17)).to(gpu)
            w = torch.rand(M, generator=torch.Generator().manual_seed(18)).to(gpu)
            loss, dlogits, accum = H.weighted_ce_forward(randn(16, M, K + 1) * 4, gt, w, True)
            return {"loss": loss, "dlogits": dlogits, "accum": accum}

        yield "front/gemm_nt_split_k/bf16", split_k(False)
        yield "front/gemm_nt_split_k/bf16x2", split_k(True)
        yield "front/gemm_mx_tail_split", mx_tail
        yield "front/gemm_tn/every_tile_split", tn(16384, 512, 1024)  # 8 tiles x 8 slices
        yield "front/gemm_tn/tail_split", tn(4096, 256 * 17, 256 * 16)  # 272 tiles = 256 + 16 split
        yield "front/gemm_tn_sgd", tn_sgd
        yield "front/mask_transpose_colsum", colsum
        yield "front/weighted_ce_forward", ce

    def rpn_head_conv(self):
        from wsovod_amd.layers import hip_ops as H
        from wsovod_amd.modeling.backbone import Conv2d, hip_conv

        if "rpn" not in self.models:
            torch.manual_seed(5)
            conv = Conv2d(512, 512, 3, stride=1, padding=1, bias=True).to(self.gpu)
            torch.nn.init.normal_(conv.weight, std=0.01)
            torch.nn.init.normal_(conv.bias, std=0.1)
            self.models["rpn"] = conv
        conv = self.models["rpn"]
        x = torch.relu(self.fixed_random(torch.empty(2, 12, 16, 512)))
        with torch.no_grad(), H.x3_mode(self.P.of("parity").x3):
            xe = H.x2_encode(x.view(-1, 512)).view(x.shape)
            return {"h": hip_conv(xe, conv, relu=True, out_fp32=True)}

    def grads(self, freeze_at, precision, wgrad_patch_bytes=None):
        def run():
            old = set_everywhere("WGRAD_PATCH_BYTES", wgrad_patch_bytes) if wgrad_patch_bytes is not None else None
            try:
                import warnings

                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    bb, out = self.forward("R18", precision, 2, freeze_at)
                    res5 = out["res5"]
                    for p in bb.parameters():
                        p.grad = None
                    (res5.float() * self.fixed_random(res5)).sum().backward()
                got = {"res5": res5.detach().permute(0, 2, 3, 1)}
                for name, p in bb.named_parameters():
                    if p.grad is not None:
                        got["d " + name] = p.grad
                assert len(got) > 1
                return got
            finally:
                if old is not None:
                    restore("WGRAD_PATCH_BYTES", old)
        return run


def run(out_path):
    from wsovod_amd import _lib

    gpu = torch.device("cuda", 0)
    cases = Cases(gpu)
    result = {"device": torch.cuda.get_device_name(0), "deterministic": os.environ.get("WSOVOD_DETERMINISTIC"),
              "digests": {}, "launches": {}}
    for name, thunk in cases.all():
        got = thunk()
        torch.cuda.synchronize()
        result["digests"][name] = {k: digest(v) for k, v in got.items()}
        for k, v in got.items():
            assert bool(torch.isfinite(v.float()).all()), (name, k)
        del got
    _lib.profile_enable(True)
    try:
        for name, thunk in cases.all():
            _lib.profile_reset()
            thunk()
            torch.cuda.synchronize()
            result["launches"][name] = {e["name"]: int(e["launches"]) for e in _lib.profile_collect() if e["launches"]}
    finally:
        _lib.profile_enable(False)
    text = json.dumps(result, indent=1, sort_keys=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"cases": len(result["digests"]), "tensors": sum(len(v) for v in result["digests"].values()),
                      "launches": sum(sum(v.values()) for v in result["launches"].values())}))
    return result


def compare(parent_a, parent_b, branch, out_path):
    """Entries whose digest differs between the two parent runs are not reproducible on the parent: listed, excluded.  No
    forward map may be among them.  Every other digest and every kernel's launch count must be equal on the branch."""
    a, b, c = (json.load(open(p)) for p in (parent_a, parent_b, branch))
    entries = lambda r: {(case, k): v for case, d in r["digests"].items() for k, v in d.items()}
    ea, eb, ec = entries(a), entries(b), entries(c)
    assert set(ea) == set(eb) == set(ec), "the three runs list different entries"
    unstable = sorted(k for k in ea if ea[k] != eb[k])
    forward_unstable = [k for k in unstable if not k[1].startswith("d ")]
    differ = sorted(k for k in ea if k not in unstable and ea[k] != ec[k])
    launches_differ = sorted(case for case in a["launches"]
                             if not (a["launches"][case] == b["launches"][case] == c["launches"].get(case)))
    rec = {"of": "tools/backbone_bits.py: two runs on the parent commit, one on this one, same machine",
           "device": c["device"], "cases": len(c["digests"]), "entries": len(ec),
           "not_reproducible_on_the_parent": [f"{case}: {k}" for case, k in unstable],
           "forward_maps_not_reproducible_on_the_parent": [f"{case}: {k}" for case, k in forward_unstable],
           "digests_compared": len(ea) - len(unstable), "digests_that_differ": [f"{case}: {k}" for case, k in differ],
           "kernels_launched": sorted({k for v in c["launches"].values() for k in v}),
           "launches_total": {"parent": sum(sum(v.values()) for v in a["launches"].values()),
                              "branch": sum(sum(v.values()) for v in c["launches"].values())},
           "cases_whose_launch_counts_differ": launches_differ,
           "equal": not (forward_unstable or differ or launches_differ)}
    text = json.dumps(rec, indent=1)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0 if rec["equal"] else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=3, metavar=("PARENT_A", "PARENT_B", "BRANCH"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare, args.out))
    run(args.out)
