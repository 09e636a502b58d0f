#!/usr/bin/env python3
"""Generate tests/golden/s2anet_loss*.npz from the REFERENCE's own compute_loss (models/head.py:353-646).

Run in the build container only (needs the reference tree):  python tests/golden/make_golden_loss.py
The reference's S2ANetHead(15) with imgs_size = (384, 384) is fed the reference's own head maps of
net_forward*.npz (batch 2 at 384^2: fam/odm cls + bbox, init / refine anchors).  The four map lists are leaf
tensors with requires_grad; loss.backward() gives their gradients.
  case 1: 12 gts in image 0, 5 in image 1 (sizes, angles, classes 0..14, boxes crossing the border)
  case 2: the same batch, image 1 without gts
  case 3: case 1 with fl_gamma 1.5, fl_alpha 0.25, smoothL1_beta 0.5, uneven FPN_balance, reg_balance 2,
          odm_balance 0.5
Stored: the targets (pixels), loss + loss_items of every case, the 20 map gradients and the FAM / ODM assign ids of
case 1.  DATA only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import import_reference_python, save_parts  # noqa: E402
from conftest import golden  # noqa: E402

CASE3 = dict(fl_gamma=1.5, fl_alpha=0.25, smoothL1_beta=0.5, FPN_balance=(1.0, 0.8, 1.2, 0.5, 2.0), reg_balance=2.0,
             odm_balance=0.5)
NAMES = ("fam_cls", "fam_bbox", "odm_cls", "odm_bbox")


def make_targets(rng):
    """pixel targets (image, class, x, y, w, h, angle) for a 384^2 batch of 2"""
    rows = []
    for img, n in ((0, 12), (1, 5)):
        for k in range(n):
            w, h = rng.uniform(10, 160), rng.uniform(8, 90)
            x, y = rng.uniform(20, 364), rng.uniform(20, 364)
            rows.append([img, 0, x, y, w, h, rng.uniform(-np.pi / 4, 3 * np.pi / 4)])
    t = np.array(rows, np.float32)
    t[:, 1] = rng.integers(0, 15, len(t))
    t[0, 1], t[1, 1], t[12, 1] = 0, 14, 14
    t[2, 2:5] = [5.0, 190.0, 120.0]           # crosses the left border
    t[3, 2:5] = [380.0, 378.0, 96.0]          # crosses the bottom-right corner
    t[13, 2:5] = [192.0, 2.0, 140.0]          # crosses the top
    return t


def main():
    import_reference_python()
    from models.head import S2ANetHead
    g = golden("net_forward.npz")
    L = 5
    maps = {n: [g["%s_%d" % (n, l)] for l in range(L)] for n in NAMES}
    init = [torch.from_numpy(g["init_anchors_%d" % l]) for l in range(L)]
    refine = [torch.from_numpy(g["refine_anchors_%d" % l]) for l in range(L)]
    rng = np.random.default_rng(20261016)
    targets = make_targets(rng)
    torch.manual_seed(0)
    out = {"targets": targets}

    def run(t, settings=None, keep_grads=False):
        head = S2ANetHead(15)
        head.imgs_size = (384, 384)
        for k, v in (settings or {}).items():
            setattr(head, k, v)
        leaves = {n: [torch.from_numpy(a.copy()).requires_grad_(True) for a in maps[n]] for n in NAMES}
        p = (leaves["fam_cls"], leaves["fam_bbox"], leaves["odm_cls"], leaves["odm_bbox"], init, refine)
        loss, items = head.compute_loss(p, torch.from_numpy(t))
        loss.backward()
        r = {"loss": loss.detach().numpy().astype(np.float32), "items": np.asarray(items, np.float32)}
        if keep_grads:
            for n in NAMES:
                for l in range(L):
                    gl = leaves[n][l].grad             # None: a level without positives never reached the graph
                    r["grad_%s_%d" % (n, l)] = np.zeros_like(maps[n][l]) if gl is None else gl.numpy()
            ids = head.assign_labels_fam_odm(p, torch.from_numpy(t))
            fam = torch.stack([torch.cat([ids[0][l].reshape(2, -1)[b] for l in range(L)]) for b in range(2)])
            odm = torch.stack([torch.cat([ids[3][l].reshape(2, -1)[b] for l in range(L)]) for b in range(2)])
            r["assign_ids"] = torch.stack([fam, odm]).numpy().astype(np.int64)
        return r

    r1 = run(targets, keep_grads=True)
    t2 = targets[targets[:, 0] == 0]
    r2 = run(t2)
    r3 = run(targets, CASE3)
    out["targets_case2"] = t2
    for k in ("loss", "items"):
        out["case1_" + k], out["case2_" + k], out["case3_" + k] = r1[k], r2[k], r3[k]
    out["case3_settings"] = np.array([CASE3["fl_gamma"], CASE3["fl_alpha"], CASE3["smoothL1_beta"], CASE3["reg_balance"],
                                      CASE3["odm_balance"]], np.float32)
    out["case3_fpn_balance"] = np.array(CASE3["FPN_balance"], np.float32)
    out["assign_ids"] = r1["assign_ids"]
    for n in NAMES:
        for l in range(L):
            out["grad_%s_%d" % (n, l)] = r1["grad_%s_%d" % (n, l)]
    print("case1", r1["loss"], r1["items"], "positives fam/odm", (r1["assign_ids"][0] >= 0).sum(),
          (r1["assign_ids"][1] >= 0).sum())
    print("case2", r2["loss"], r2["items"])
    print("case3", r3["loss"], r3["items"])
    save_parts("s2anet_loss", out)


if __name__ == "__main__":
    main()
