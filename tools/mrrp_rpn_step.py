"""The MRRP RPN, measured: its proposal stage with either top-k route, and the R18 MRRP model's training step with the RPN
next to the same model on precomputed proposals, in ONE process:

    python tools/mrrp_rpn_step.py [--images 1 8]      (one MI355X)

Part (a): find_top_rpn_proposals_group (top-k, decode per level, NMS per (image, level, anchor), merge, the one host read)
on the 75 x 100 map of an 800 x 600 image, L = 3 levels with the shipped per-level anchors (A = 6), pre 2048 / post 1024,
on the SAME logits and deltas (the seeded R18 MRRP model's own head outputs) with WSOVOD_RPN_TOPK = hip and = torch, the
two routes taking turns run by run; 3 warm-up + 15 timed rounds, medians with min / max (the spread).  `hip_wins`: the HIP
median is below the torch median by more than the larger of the two spreads -- the rule hip_ops.RPN_TOPK_ROUTE's default is
derived by.  The top-k alone is timed the same way.
Part (b): the eager training step (512 loaded proposals, K = 20, "parity") of hot_path_r18_mrrp_rpn.yaml next to
hot_path_r18_mrrp.yaml, interleaved step by step, the RPN model under both routes.
Writes profiles/mrrp_rpn_step.json and prints it."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from wsovod_amd.data import make_batch
from wsovod_amd.engine import build_optimizer, run_step
from wsovod_amd.layers import hip_ops as H
from wsovod_amd.modeling import proposal_generator as PG
from wsovod_amd.testing import build_hot_path_model

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


def _ab(forms, rounds, warmup):
    """forms: {route: fn}; the routes take turns, the order alternating round by round."""
    ms = {k: [] for k in forms}
    names = list(forms)
    for rnd in range(warmup + rounds):
        for name in (names if rnd % 2 == 0 else names[::-1]):
            H.RPN_TOPK_ROUTE = name
            t, _ = _timed(forms[name])
            if rnd >= warmup:
                ms[name].append(t)
    hip, tor = _stat(ms["hip"]), _stat(ms["torch"])
    spread = max(hip["ms_max"] - hip["ms_min"], tor["ms_max"] - tor["ms_min"])
    return {"hip": hip, "torch": tor, "spread_ms": round(spread, 4), "hip_wins": bool(hip["ms"] < tor["ms"] - spread)}


def stage(model, n, rounds, warmup):
    pg = model.proposal_generator
    L, A = pg.mrrp_num_branch, pg.rpn_head.num_anchors
    with torch.no_grad():
        feat = torch.relu(torch.randn(L * n, 512, HH, WW, device="cuda")).contiguous(memory_format=torch.channels_last)
        anchors = pg.anchor_generator([feat] * L)
        lo, de = pg.rpn_head.forward_nhwc(feat, num_images=n)
        logits, deltas = list(lo.view(L, n, -1).unbind(0)), list(de.view(L, n, -1, 4).unbind(0))
        sizes = [(600, 800)] * n
        k = min(HH * WW, pg.pre_nms_topk[True])
        stacked = torch.stack(logits).view(L * n, HH * WW, A)

        def whole():
            return PG.find_top_rpn_proposals_group(anchors, logits, deltas, sizes, [A] * L, pg.box2box_transform, pg.nms_thresh,
                                                   pg.pre_nms_topk[True], pg.post_nms_topk[True], pg.min_box_size, False)

        kept = [len(p) for p in whole()]
        return {"kept_per_image": kept,
                "stage": _ab({"hip": whole, "torch": whole}, rounds, warmup),
                "topk_alone": _ab({"hip": lambda: PG.rpn_group_topk(stacked, k), "torch": lambda: PG.rpn_group_topk(stacked, k)},
                                  rounds, warmup)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--proposals", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "mrrp_rpn_step.json"))
    args = ap.parse_args()
    default_route = H.RPN_TOPK_ROUTE
    cfg, rpn_model = build_hot_path_model(seed=0, depth=18, mrrp=True, rpn=True, precision="parity", device="cuda:0")
    cfg_p, pre_model = build_hot_path_model(seed=0, depth=18, mrrp=True, precision="parity", device="cuda:0")
    out = {"note": "nobody had measured this before; no target was set", "device": torch.cuda.get_device_name(0),
           "proposal_stage": {"of": f"find_top_rpn_proposals_group, L = 3, A = 6, {HH} x {WW} map (800 x 600 image), pre 2048 / post "
                                    f"1024, routes interleaved, {args.warmup} warm-up + {args.rounds} timed rounds, medians (min - max)"}}
    torch.manual_seed(0)
    for n in args.images:
        out["proposal_stage"][f"{n} images"] = stage(rpn_model, n, args.rounds, args.warmup)
    torch.cuda.empty_cache()
    runs = []
    for name, (c, m), route in (("rpn, top-k hip", (cfg, rpn_model), "hip"), ("rpn, top-k torch", (cfg, rpn_model), "torch"),
                                ("precomputed proposals", (cfg_p, pre_model), "torch")):
        c.SOLVER.BASE_LR = 1e-4
        m.train()
        runs.append({"name": name, "model": m, "route": route, "opt": build_optimizer(c, m)})
    out["step"] = {"of": f"eager training step (run_step), R18 MRRP, parity, 800x600 x {args.proposals} loaded proposals, K = 20, "
                         f"models interleaved step by step, {args.warmup} warm-up + {args.rounds} timed steps, medians"}
    for n in args.images:
        host = make_batch(n, args.proposals, 20, seed=123)
        batch = [{"image": x["image"].to("cuda"), "proposals": x["proposals"].to("cuda"), "instances": x["instances"],
                  "height": x["height"], "width": x["width"]} for x in host]
        ms = {r["name"]: [] for r in runs}

        def one_step(r):
            H.RPN_TOPK_ROUTE = r["route"]
            return run_step(r["model"], r["opt"], batch)

        for rnd in range(args.warmup + args.rounds):
            for r in runs[rnd % len(runs):] + runs[:rnd % len(runs)]:
                t, losses = _timed(lambda: one_step(r))
                assert all(bool(torch.isfinite(v)) for v in losses.values()), (r["name"], losses)
                if rnd >= args.warmup:
                    ms[r["name"]].append(t)
        out["step"][f"{n} images"] = {k: {**_stat(v), "images_per_s": round(n / statistics.median(v) * 1e3, 2)} for k, v in ms.items()}
    H.RPN_TOPK_ROUTE = default_route
    wins = [out["proposal_stage"][f"{n} images"]["stage"]["hip_wins"] for n in args.images]
    out["default_route"] = {"rule": "hip when the stage's HIP median is below torch's by more than the larger spread at every size",
                            "derived": "hip" if all(wins) else "torch"}
    text = json.dumps(out, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
