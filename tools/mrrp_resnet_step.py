"""The MRRP ResNets' res5, measured: one launch over all branches against one launch per branch, and the MRRP models'
training step next to the plain ResNet models', in ONE process:

    python tools/mrrp_resnet_step.py [--images 1 4 8 32] [--step-images 8 1]      (one MI355X)

Part (a): the res5 stage of R18 (two MRRPBasicBlocks, 256 -> 512) and R50 (three MRRPBottleneckBlocks, 1024 -> 2048) with
dilations 1 / 2 / 4 on the res4 map of an 800 x 600 image (75 x 100), with WSOVOD_BRANCH_BATCHED = 1 and = 0 on the SAME
operands and weights, for f16mx ("parity_mx") and bf16x2 ("parity"), the two forms taking turns run by run; 3 warm-up + 15
timed rounds, medians with min / max (the spread).  `one_launch_wins`: the one-launch median is below the loop's by more than
the larger of the two spreads -- the rule BATCHED_UP_TO of modeling/backbone_resnet_mrrp.py is derived by.
Part (b): the HotPathTrainer step (512 proposals, K = 20) of the MRRP models in "parity" and "parity_mx" next to the plain
ResNet models', interleaved step by step.  Writes profiles/mrrp_resnet_step.json and prints it."""
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
from wsovod_amd.modeling.backbone_resnet_mrrp import MRRPBasicBlock, MRRPBottleneckBlock
from wsovod_amd.testing import build_hot_path_model

DILATIONS = (1, 2, 4)
HH, WW = 75, 100


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def _stat(ms):
    return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def res5_stage(gpu, depth):
    kw = dict(norm="FrozenBN", num_branch=3, dilations=DILATIONS)
    if depth == 18:
        blocks = [MRRPBasicBlock(256 if i == 0 else 512, 512, shared_input=i == 0, **kw) for i in range(2)]
    else:
        blocks = [MRRPBottleneckBlock(1024 if i == 0 else 2048, 2048, bottleneck_channels=512, shared_input=i == 0, **kw) for i in range(3)]
    blocks[-1]._emits_fp32 = True
    return torch.nn.Sequential(*blocks).to(gpu).eval()


def res5_forms(gpu, stage, cin, n, fmt, rounds, warmup):
    x = torch.relu(torch.randn(n, HH, WW, cin, device=gpu))
    ms = {"1": [], "0": []}
    with torch.no_grad(), P.scope(P.of("parity_mx" if fmt == "f16mx" else "parity"), mx=fmt == "f16mx"):
        xin = H.x2_encode(x.view(-1, cin)).view(x.shape)
        if fmt == "f16mx":
            xin = H.mx_from_x2(xin)
        del x
        for rnd in range(warmup + rounds):
            for form in (("1", "0") if rnd % 2 == 0 else ("0", "1")):
                os.environ["WSOVOD_BRANCH_BATCHED"] = form
                t, y = _timed(lambda: stage(xin))
                del y
                if rnd >= warmup:
                    ms[form].append(t)
    os.environ.pop("WSOVOD_BRANCH_BATCHED", None)
    one, loop = _stat(ms["1"]), _stat(ms["0"])
    spread = max(one["ms_max"] - one["ms_min"], loop["ms_max"] - loop["ms_min"])
    return {"one_launch": one, "loop": loop, "spread_ms": round(spread, 4), "one_launch_wins": bool(one["ms"] < loop["ms"] - spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[1, 4, 8, 32])
    ap.add_argument("--step-images", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--depths", type=int, nargs="+", default=[18, 50])
    ap.add_argument("--proposals", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "mrrp_resnet_step.json"))
    args = ap.parse_args()
    gpu = torch.device("cuda", 0)
    out = {"note": "nobody had measured this before; no target was set",
           "device": torch.cuda.get_device_name(0),
           "res5": {"of": f"the whole res5 stage (R18: 2 MRRPBasicBlocks, R50: 3 MRRPBottleneckBlocks), dilations {list(DILATIONS)}, "
                          f"{HH} x {WW} map (800 x 600 image), forms interleaved, {args.warmup} warm-up + {args.rounds} timed rounds, "
                          "medians (min - max)"}}
    torch.manual_seed(0)
    for depth in args.depths:
        stage, cin = res5_stage(gpu, depth), 256 if depth == 18 else 1024
        for fmt in ("f16mx", "bf16x2"):
            out["res5"][f"R{depth} {fmt}"] = {f"{n} images": res5_forms(gpu, stage, cin, n, fmt, args.rounds, args.warmup)
                                               for n in args.images}
        del stage
    torch.cuda.empty_cache()
    runs = []
    for depth in args.depths:
        for precision in ("parity_mx", "parity"):
            for mrrp in (True, False):
                cfg, model = build_hot_path_model(seed=0, depth=depth, mrrp=mrrp, precision=precision, device="cuda:0")
                cfg.SOLVER.BASE_LR = 1e-4
                model.train()
                runs.append({"name": f"R{depth} {precision} {'mrrp' if mrrp else 'plain'}",
                             "trainer": HotPathTrainer(model, build_optimizer(cfg, model))})
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
