"""The MRRP VGG16 backbone's plain5, measured: one launch over all branches against one launch per branch, and the MRRP
model's training step next to the plain VGG16's, in ONE process:

    python tools/mrrp_vgg_step.py [--images 1 4 8 32] [--step-images 8 1]      (one MI355X)

Part (a): the three convs of plain5 (512 -> 512, 3x3, dilations 1 / 2 / 4, conv1 on the shared input) on plain5's map of an
800 x 600 image (74 x 99), as `hip_conv_branches(..., batched=True)` and `batched=False` on the SAME operands, for f16mx
("parity_mx") and bf16x2 ("parity"), the two forms taking turns launch by launch; 3 warm-up + 15 timed rounds, medians with
min / max (the spread).  `one_launch_wins`: the batched median is below the loop's by more than the larger of the two spreads.
Part (b): the HotPathTrainer step (512 proposals, K = 20) of the MRRP model in "parity" and "parity_mx" next to the plain
VGG16 model's, interleaved step by step.  Writes profiles/mrrp_vgg_step.json and prints it."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from wsovod_amd.data import make_batch
from wsovod_amd.engine import HotPathTrainer, build_optimizer
from wsovod_amd.layers import hip_ops as H, precision as P
from wsovod_amd.modeling.backbone import Conv2d
from wsovod_amd.modeling.backbone_vgg_mrrp import hip_conv_branches
from wsovod_amd.testing import build_hot_path_model

DILATIONS = (1, 2, 4)
HH, WW, CH = 74, 99, 512


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def _stat(ms):
    return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def plain5_forms(gpu, n, fmt, rounds, warmup):
    convs = []
    for _ in range(3):
        c = Conv2d(CH, CH, 3, padding=1, bias=True).to(gpu)
        torch.nn.init.normal_(c.weight, std=0.02)
        convs.append(c)
    x = torch.relu(torch.randn(n, HH, WW, CH, device=gpu))
    rec = P.of("parity_mx" if fmt == "f16mx" else "parity")
    ms = {True: [], False: []}
    with torch.no_grad(), P.scope(rec, mx=fmt == "f16mx"):
        xin = H.x2_encode(x.view(-1, CH)).view(x.shape)
        if fmt == "f16mx":
            xin = H.mx_from_x2(xin)

        def block(batched):
            y = xin
            for j, c in enumerate(convs):
                y = hip_conv_branches(y, c, DILATIONS, shared_input=j == 0, relu=True, out_fp32=j == 2, batched=batched)
            return y

        for rnd in range(warmup + rounds):
            for batched in ((True, False) if rnd % 2 == 0 else (False, True)):
                t, y = _timed(lambda: block(batched))
                del y
                if rnd >= warmup:
                    ms[batched].append(t)
    one, loop = _stat(ms[True]), _stat(ms[False])
    spread = max(one["ms_max"] - one["ms_min"], loop["ms_max"] - loop["ms_min"])
    tiles = -(-n * HH * WW // 256) * 2
    return {"one_launch": one, "loop": loop, "spread_ms": round(spread, 4), "workgroups_per_single_launch": tiles,
            "workgroups_per_batched_launch": tiles * len(DILATIONS), "one_launch_wins": bool(one["ms"] < loop["ms"] - spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[1, 4, 8, 32])
    ap.add_argument("--step-images", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--proposals", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "mrrp_vgg_step.json"))
    args = ap.parse_args()
    gpu = torch.device("cuda", 0)
    out = {"note": "nobody had measured this before; no target was set",
           "device": torch.cuda.get_device_name(0),
           "plain5_convs": {"of": f"three 512 -> 512 3x3 convs, dilations {list(DILATIONS)}, {HH} x {WW} map (800 x 600 image), forms "
                                  f"interleaved, {args.warmup} warm-up + {args.rounds} timed rounds, medians (min - max)"}}
    for fmt in ("f16mx", "bf16x2"):
        out["plain5_convs"][fmt] = {f"{n} images": plain5_forms(gpu, n, fmt, args.rounds, args.warmup) for n in args.images}
    runs = []
    for precision in ("parity_mx", "parity"):
        for mrrp in (True, False):
            cfg, model = build_hot_path_model(seed=0, backbone="vgg16", mrrp=mrrp, precision=precision, device="cuda:0")
            cfg.SOLVER.BASE_LR = 1e-4
            model.train()
            runs.append({"name": f"{precision} {'mrrp' if mrrp else 'plain'}", "trainer": HotPathTrainer(model, build_optimizer(cfg, model))})
    out["step"] = {"of": f"HotPathTrainer step, 800x600 x {args.proposals} proposals, K = 20, models interleaved step by step, "
                         f"{args.warmup} warm-up + {args.rounds} timed steps, medians"}
    for n in args.step_images:
        host = make_batch(n, args.proposals, 20, seed=123)
        batch = [{"image": x["image"].to(gpu), "proposals": x["proposals"].to(gpu), "instances": x["instances"],
                  "height": x["height"], "width": x["width"]} for x in host]
        ms = {r["name"]: [] for r in runs}

        def one_step(r):
            losses = r["trainer"].run_step(batch)
            r["trainer"].flush()
            return losses

        for rnd in range(args.warmup + args.rounds):
            for r in runs[rnd % len(runs):] + runs[:rnd % len(runs)]:
                t, losses = _timed(lambda: one_step(r))
                assert all(bool(torch.isfinite(v)) for v in losses.values()), (r["name"], losses)
                if rnd >= args.warmup:
                    ms[r["name"]].append(t)
        out["step"][f"{n} images"] = {k: {**_stat(v), "images_per_s": round(n / statistics.median(v) * 1e3, 2)} for k, v in ms.items()}
    for r in runs:
        r["trainer"].close()
    text = json.dumps(out, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
