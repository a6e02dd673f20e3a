"""Generate tests/golden/g23_mrrp_rpn.npz by running the REFERENCE's own WSOVODRPN_V2(mrrp_on=True),
find_top_rpn_proposals_group and the RPN branch of its meta-architecture on one training step, loaded by path over the
stand-in modules of make_golden.py exactly as g12 was made (brute-force batched_nms, first-k anchor sub-sampling).

    python tests/golden/make_golden_mrrp_rpn.py

R18 MRRP (branch dilations [1, 2, 4]) with the per-level anchor SIZES of the shipped config, two 256 x 352 images with 40
loaded boxes each, K = 20, seeded weights in the manner of shapes_rpn_r18.npz (the MRRP model has the same state-dict
keys and shapes).  The loaded boxes' level ids are drawn by a seeded torch.randint and stored.  The deltas of all three levels
(what the proposals are decoded from: the CPU restatement needs every one, k = H*W here) go to a second file,
g23_mrrp_rpn_deltas.npz, so that each file stays below the largest fixture already committed; g23 itself keeps a strided sample."""
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden import gen  # noqa: E402
from tests.golden import make_golden as MG  # noqa: E402

SEED_WEIGHTS, SEED_IDS = 41, 45
SEED_BATCHES = (44, 46, 47, 48, 49)  # the first whose anchor labels survive a 1e-2 px move of the pseudo-GT boxes is kept (g12's 43: 132 flip)


def labels_are_robust(cfg, anchors, logits, gt, labels_ref):
    """fp32 on the device reproduces the pseudo-GT boxes to ~5e-3 px (the targets' bar is 1e-2): a fixture whose anchor labels
    flip under such a move (a row of equal anchors tying for a wide box's best IoU) cannot be held to 4 label differences."""
    from tests import mrrp_rpn_util as U
    from wsovod_amd.modeling.box_regression import Box2BoxTransform
    from wsovod_amd.modeling.matcher import Matcher

    worst = 0
    draw = torch.Generator().manual_seed(1)
    for _ in range(8):
        moved = [b + (torch.rand(b.shape, generator=draw) * 2 - 1) * 1e-2 for b in gt]
        zeros = [torch.zeros(l.shape + (4,)) for l in logits]
        lab = U.rpn_losses(anchors, logits, zeros, moved, Box2BoxTransform(weights=cfg.MODEL.RPN.BBOX_REG_WEIGHTS),
                           Matcher(cfg.MODEL.RPN.IOU_THRESHOLDS, cfg.MODEL.RPN.IOU_LABELS, allow_low_quality_matches=True),
                           gen.first_k_subsample, 512, 0.5)[2]
        worst = max(worst, int((lab.to(labels_ref.dtype) != labels_ref).sum()))
    print("label changes under a 1e-2 px move of the targets:", worst)
    return worst <= 2


def main():
    r = MG.load_reference()
    MG._install_rpn(r)
    MG._mod("detectron2.layers.wrappers", _NewEmptyTensorOp=None)
    MG.load_ref("wsovod.modeling.backbone.mrrp_conv", "wsovod/modeling/backbone/mrrp_conv.py")
    MG.load_ref("wsovod.modeling.backbone.resnet_wsl_mrrp", "wsovod/modeling/backbone/resnet_wsl_mrrp.py")
    for seed in SEED_BATCHES:
        if one(r, seed):
            return
    raise SystemExit("no robust seed")


def one(r, SEED_BATCH):
    from wsovod_amd.testing import hot_path_cfg

    import pickle
    import tempfile

    K, D = 20, 512
    emb = os.path.join(tempfile.mkdtemp(prefix="golden_"), "emb.pkl")
    with open(emb, "wb") as f:
        pickle.dump(torch.randn(K, D), f)
    cfg = hot_path_cfg(depth=18, K=K, D=D, device="cpu", weight_path=emb, rpn=True, mrrp=True)
    assert cfg.MODEL.ANCHOR_GENERATOR.SIZES == [[32, 64], [128, 256], [512, 768]] and cfg.MODEL.HIP.MRRP_RPN
    cfg.MODEL.PIXEL_STD = list(gen.PIXEL_STD)
    cfg.MODEL.ROI_HEADS.NAME = "WSOVODROIHeads"
    cfg.DATASETS.TRAIN = ("synthetic",)
    cfg.SOLVER.MAX_ITER = 4000
    torch.manual_seed(0)
    model = r.meta.GeneralizedRCNN_WSOVOD(cfg)
    pgm = model.proposal_generator
    assert type(pgm).__name__ == "WSOVODRPN_V2" and pgm.mrrp_on and model.roi_heads.rpn_on
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(gen.seeded_state(shapes, seed=SEED_WEIGHTS), strict=True)
    model.train()
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = 1e-12
    arrays = {"keys": np.array(list(shapes.keys())), "shapes": np.array([str(v) for v in shapes.values()]),
              "batch_seed": np.array(SEED_BATCH)}
    inputs = MG.to_inputs(gen.seeded_batch(2, 40, K, 256, 352, seed=SEED_BATCH))
    captured = {"ids": []}
    orig = pgm.predict_proposals

    def cap_props(*a, **k):
        o = orig(*a, **k)
        captured["proposals"] = [(p.proposal_boxes.tensor.clone(), p.objectness_logits.clone(), p.level_ids.clone()) for p in o]
        return o

    pgm.predict_proposals = cap_props
    orig_label = pgm.label_and_sample_anchors

    def cap_label(*a, **k):
        o = orig_label(*a, **k)
        captured["anchor_labels"] = torch.stack(o[0])
        return o

    pgm.label_and_sample_anchors = cap_label
    real_randint = torch.randint
    draw = torch.Generator().manual_seed(SEED_IDS)

    def seeded_randint(low, high, size, **kw):  # the meta-architecture's draw of the loaded boxes' level ids
        ids = real_randint(int(low), int(high), size, generator=draw, dtype=torch.int64)
        captured["ids"].append(ids.clone())
        return ids

    torch.randint = seeded_randint
    try:
        loss_dict = model(inputs)
    finally:
        torch.randint = real_randint
    sum(loss_dict.values()).backward()
    for k, v in loss_dict.items():
        arrays[f"loss/{k}"] = v
    L = len(pgm.pred_objectness_logits)
    assert L == 3 and len(captured["ids"]) == 2
    for l in range(L):
        arrays[f"rpn_logits{l}"] = pgm.pred_objectness_logits[l]
    all_deltas = torch.cat(pgm.pred_anchor_deltas, dim=1)  # (N, L*H*W*A, 4)
    arrays["rpn_deltas_sample"] = gen.strided_sample(all_deltas, 8192)
    for i, (bx, sc, ids) in enumerate(captured["proposals"]):
        arrays[f"prop{i}/boxes"], arrays[f"prop{i}/logits"], arrays[f"prop{i}/level_ids"] = bx, sc, ids
        arrays[f"loaded{i}/level_ids"] = captured["ids"][i]
    arrays["anchor_labels"] = captured["anchor_labels"]
    for i, t in enumerate(model.roi_heads.proposal_targets):
        arrays[f"target{i}/gt_boxes"] = t.gt_boxes.tensor
        arrays[f"target{i}/gt_classes"] = t.gt_classes
    for k, q in model.named_parameters():
        if q.requires_grad:
            arrays["gradnorm/" + k] = q.grad.double().norm() if q.grad is not None else torch.tensor(-1.0)
    print({k: float(v) for k, v in loss_dict.items()}, [len(p[0]) for p in captured["proposals"]],
          [sorted(set(p[2].tolist())) for p in captured["proposals"]])
    if not labels_are_robust(cfg, [a.tensor for a in pgm.anchors], [l.detach() for l in pgm.pred_objectness_logits],
                             [t.gt_boxes.tensor for t in model.roi_heads.proposal_targets], captured["anchor_labels"]):
        return False
    MG.save("g23_mrrp_rpn", **arrays)
    MG.save("g23_mrrp_rpn_deltas", **{f"rpn_deltas{l}": pgm.pred_anchor_deltas[l] for l in range(L)})
    print(SEED_BATCH, os.path.getsize(os.path.join(HERE, "g23_mrrp_rpn.npz")))
    return True


if __name__ == "__main__":
    main()
