"""Generates tests/golden/ref_box_losses.npz by running the REFERENCE's own box-regression losses on seeded inputs:
_dense_box_regression_loss (modeling/box_regression.py:229-270) and FastRCNNOutputLayers.box_reg_loss (the CLIP-era class,
modeling/roi_heads/fast_rcnn.py:646-689), both over its Box2BoxTransform, in f32 with torch autograd.  Reuses the make_golden.py
harness (reference leaf modules imported with their package __init__s bypassed).  fvcore is not installed: giou_loss and
smooth_l1_loss are supplied here as independent statements of their published definitions (not taken from oracle/, so the
comparison is not circular).  Only data is written: inputs, losses and gradients.

Cases: both loss types for the RPN and the box head, beta 1/9 and 1.0, an image without ground truth, rows with dw / dh above the
clamp, disjoint, overlapping and exactly matching boxes (the constructed rows of tests/exact_box_losses.py come first).

usage:  python tests/golden/make_golden_box_losses.py
"""
import importlib
import os
import sys

import numpy as np
import torch

import make_golden as mg

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import exact_box_losses as B  # noqa: E402
import exact_losses as E  # noqa: E402


def giou_loss(boxes1, boxes2, reduction="none", eps=1e-7):
    """fvcore.nn.giou_loss (published definition; Generalized IoU, arXiv:1902.09630)"""
    x1, y1, x2, y2 = boxes1.unbind(dim=-1)
    x1g, y1g, x2g, y2g = boxes2.unbind(dim=-1)
    assert (x2 >= x1).all() and (y2 >= y1).all()
    xkis1, ykis1 = torch.max(x1, x1g), torch.max(y1, y1g)
    xkis2, ykis2 = torch.min(x2, x2g), torch.min(y2, y2g)
    intsctk = torch.zeros_like(x1)
    mask = (ykis2 > ykis1) & (xkis2 > xkis1)
    intsctk[mask] = (xkis2[mask] - xkis1[mask]) * (ykis2[mask] - ykis1[mask])
    unionk = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g) - intsctk
    iouk = intsctk / (unionk + eps)
    xc1, yc1 = torch.min(x1, x1g), torch.min(y1, y1g)
    xc2, yc2 = torch.max(x2, x2g), torch.max(y2, y2g)
    area_c = (xc2 - xc1) * (yc2 - yc1)
    miouk = iouk - ((area_c - unionk) / (area_c + eps))
    loss = 1 - miouk
    return loss.sum() if reduction == "sum" else loss.mean() if reduction == "mean" else loss


N, R_RPN, R_BOX, K = 3, 40, 64, 5
LOSSES = (("giou", "giou", 0.0), ("sl1_b0.111", "smooth_l1", 1.0 / 9), ("sl1_b1", "smooth_l1", 1.0))


def main():
    mg.setup()
    importlib.import_module("fvcore.nn").giou_loss = giou_loss
    br = importlib.import_module("detectron2.modeling.box_regression")
    fr = importlib.import_module("detectron2.modeling.roi_heads.fast_rcnn")
    S, L = sys.modules["detectron2.structures"], sys.modules["detectron2.layers"]
    assert br.giou_loss is giou_loss and br.smooth_l1_loss is mg.smooth_l1_loss and fr.giou_loss is giou_loss
    out = {}
    # ---- RPN: _dense_box_regression_loss over N images of R anchors; image 1 has no ground truth (an all-false mask, zero boxes)
    w = B.RPN_W
    for tag, loss_type, beta in LOSSES:
        b2b = br.Box2BoxTransform(weights=w)
        cb, cg, cd = B.constructed_rows(w)
        anchors = E._boxes(R_RPN, 401)
        anchors[:B.NCON] = cb
        gt = torch.stack([E._boxes(R_RPN, 402), torch.zeros(R_RPN, 4), E._boxes(R_RPN, 403)])
        gt[0, :B.NCON] = cg
        deltas = B._deltas(N * R_RPN, w, 404).view(N, R_RPN, 4)
        deltas[0, :B.NCON] = cd
        fg = torch.rand((N, R_RPN), generator=E._g(405)) < 0.6
        fg[0, :B.NCON], fg[1] = True, False
        if loss_type == "smooth_l1":                                    # a third of the rows within beta of their target
            near = torch.zeros_like(fg)
            near[:, B.NCON::3] = True
            for i in (0, 2):
                tg = b2b.get_deltas(anchors, gt[i])
                deltas[i][near[i]] = (tg + E._randn((R_RPN, 4), 406 + i, 0.05))[near[i]]
        deltas.requires_grad_(True)
        loss = br._dense_box_regression_loss([S.Boxes(anchors)], b2b, [deltas], [g for g in gt], fg, box_reg_loss_type=loss_type,
                                             smooth_l1_beta=beta)
        loss.backward()
        name = f"rpn_{tag}"
        out.update({f"{name}/anchors": anchors.numpy(), f"{name}/gt": gt.numpy(), f"{name}/deltas": deltas.detach().numpy(),
                    f"{name}/fg": fg.numpy(), f"{name}/loss": loss.detach().numpy(), f"{name}/grad": deltas.grad.numpy(),
                    f"{name}/beta": np.float64(beta), f"{name}/weights": np.asarray(w, dtype=np.float64), f"{name}/ncon": np.int64(B.NCON)})
        print(name, float(loss.detach()), int(fg.sum()))
    # ---- box head: FastRCNNOutputLayers.box_reg_loss, class-specific deltas, background rows (class K)
    w = B.BOX_W
    for tag, loss_type, beta in LOSSES:
        b2b = br.Box2BoxTransform(weights=w)
        pred = fr.FastRCNNOutputLayers(L.ShapeSpec(channels=16, height=1, width=1), box2box_transform=b2b, num_classes=K,
                                       smooth_l1_beta=beta, box_reg_loss_type=loss_type, bg_cls_loss_weight=None,
                                       openset_test=(None, None, 0.01, 0.5), loss_weight={"loss_box_reg": 1.0})
        cb, cg, cd = B.constructed_rows(w)
        g = E._g(411)
        prop, gtb = E._boxes(R_BOX, 412), E._boxes(R_BOX, 413)
        prop[:B.NCON], gtb[:B.NCON] = cb, cg
        cls = torch.randint(0, K, (R_BOX,), generator=g)
        cls[torch.rand(R_BOX, generator=g) < 0.4] = K                   # background
        cls[:B.NCON] = torch.arange(B.NCON) % K
        deltas = E._randn((R_BOX, 4 * K), 414)
        own = B._deltas(R_BOX, w, 415)
        if loss_type == "smooth_l1":
            tg = b2b.get_deltas(prop, gtb)
            own[B.NCON::3] = (tg + E._randn((R_BOX, 4), 416, 0.05))[B.NCON::3]
        own[:B.NCON] = cd
        fgr = torch.nonzero(cls < K)[:, 0]
        deltas[fgr[:, None], 4 * cls[fgr][:, None] + torch.arange(4)[None, :]] = own[fgr]
        deltas.requires_grad_(True)
        loss = pred.box_reg_loss(prop, gtb, deltas, cls)
        loss.backward()
        name = f"box_{tag}"
        out.update({f"{name}/proposals": prop.numpy(), f"{name}/gt": gtb.numpy(), f"{name}/deltas": deltas.detach().numpy(),
                    f"{name}/classes": cls.numpy(), f"{name}/loss": loss.detach().numpy(), f"{name}/grad": deltas.grad.numpy(),
                    f"{name}/beta": np.float64(beta), f"{name}/weights": np.asarray(w, dtype=np.float64), f"{name}/ncon": np.int64(B.NCON)})
        print(name, float(loss.detach()), int(fgr.numel()))
    path = os.path.join(mg.HERE, "ref_box_losses.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
