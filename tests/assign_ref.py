"""CPU restatements of the reference's training-target side, used by the assign tests.

* `assign_frame`: AnchorAssigner.assign (anchor_assigner.py:337-457) vectorised in numpy.  `typing="f32"` keeps every IoU
  intermediate in float32 (the reference run as plain Python under numpy >= 2, which is how the goldens are made and what the GPU
  computes); `typing="f64"` is what real numba compiles iou_jit to: `+ eps` with a float64 argument lifts iw, ih, the areas and the
  quotient to double, and only the store rounds to float32.
* `loss_terms` / `batch_loss`: LossGenerator.generate (loss_generator.py:26-253, NormByNumPositives) restated in torch on the CPU,
  per frame and for a batch; `metric_counts`: _calc_binary_metrics (metrics.py:55-69) at the four thresholds.
"""
import numpy as np
import torch

F32 = np.float32
THRESHOLDS = (0.1, 0.3, 0.5, 0.7)


def near_bv(boxes):
    """rbbox2d_to_near_bbox (box_np_ops.py:308-331) of f32[N,7] boxes, float32 throughout."""
    boxes = np.asarray(boxes, dtype=F32)
    r = boxes[:, 6]
    pi = F32(np.pi)
    lp = np.abs(r - np.floor(r / pi + F32(0.5)) * pi)
    sw = lp > F32(np.pi / 4)
    dx = np.where(sw, boxes[:, 4], boxes[:, 3])
    dy = np.where(sw, boxes[:, 3], boxes[:, 4])
    return np.stack([boxes[:, 0] - dx / F32(2), boxes[:, 1] - dy / F32(2), boxes[:, 0] + dx / F32(2), boxes[:, 1] + dy / F32(2)], 1)


def iou(a, g, typing="f32"):
    """iou_jit(a, g, eps=0.0) -> f32[len(a), len(g)]."""
    a = a[:, None, :]
    g = g[None, :, :]
    iw = np.minimum(a[..., 2], g[..., 2]) - np.maximum(a[..., 0], g[..., 0])
    ih = np.minimum(a[..., 3], g[..., 3]) - np.maximum(a[..., 1], g[..., 1])
    if typing == "f64":
        iw, ih = iw.astype(np.float64), ih.astype(np.float64)
        aa = (a[..., 2] - a[..., 0]).astype(np.float64) * (a[..., 3] - a[..., 1]).astype(np.float64)
        ga = (g[..., 2] - g[..., 0]).astype(np.float64) * (g[..., 3] - g[..., 1]).astype(np.float64)
    else:
        aa = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
        ga = (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])
    inter = iw * ih
    with np.errstate(divide="ignore", invalid="ignore"):
        v = inter / ((aa + ga) - inter)
    return np.where((iw > 0) & (ih > 0), v, 0).astype(F32)


def box_encode(boxes, anchors):
    """box_encode (box_np_ops.py:366-382), float32 numpy."""
    xa, ya, za, la, wa, ha, ra = np.split(anchors, 7, axis=-1)
    xg, yg, zg, lg, wg, hg, rg = np.split(boxes, 7, axis=-1)
    diagonal = np.sqrt(la ** 2 + wa ** 2)
    return np.concatenate([(xg - xa) / diagonal, (yg - ya) / diagonal, (zg - za) / ha, np.log(lg / la), np.log(wg / wa), np.log(hg / ha),
                           rg - ra], axis=-1)


def assign_frame(anchors, anchors_bv, class_masks, thr_m, thr_u, gt, gt_cls, mask, typing="f32"):
    """-> dict(labels i32[A], bbox_targets f32[A,7], outside_w f32[A], dir_targets i32[A], forced bool[A], max f32[A] (NaN where
    not computed), ties: number of (box, anchor) pairs at a box maximum beyond the first per box)."""
    A = anchors.shape[0]
    gt = np.asarray(gt, dtype=F32).reshape(-1, 7)
    gt_cls = np.asarray(gt_cls).reshape(-1)
    mask = np.asarray(mask).astype(bool)
    labels = -np.ones(A, np.int32)
    tgt = np.zeros((A, 7), F32)
    forced = np.zeros(A, bool)
    amax = np.full(A, np.nan, F32)
    ties = 0
    for ci, (s, e) in enumerate(class_masks):
        g = gt[gt_cls == ci + 1]
        inside = np.nonzero(mask[s:e])[0] + s
        if len(g) == 0 or len(inside) == 0:
            labels[inside] = 0
            continue
        ov = iou(anchors_bv[inside], near_bv(g), typing)
        arg = ov.argmax(1)
        mx = ov[np.arange(len(inside)), arg]
        gmax = ov.max(0)
        gmax[gmax == 0] = -1
        hit = ov == gmax
        ties += int(np.maximum(hit.sum(0) - 1, 0).sum())
        fo = hit.any(1)
        # anchor_assigner.py:381-392: forced -> 1, pos (>= matched) -> 1, bg (< unmatched) -> 0 overwrites, forced -> 1 again
        lab = -np.ones(len(inside), np.int32)
        lab[mx >= F32(thr_m[ci])] = 1
        lab[mx < F32(thr_u[ci])] = 0
        lab[fo] = 1
        labels[inside] = lab
        forced[inside] = fo
        amax[inside] = mx
        pos = lab == 1
        tgt[inside[pos]] = box_encode(g[arg[pos]], anchors[inside[pos]])
    ow = (labels > 0).astype(F32)
    dirt = ((tgt[:, 6] + anchors[:, 6]) > 0).astype(np.int32)
    return dict(labels=labels, bbox_targets=tgt, outside_w=ow, dir_targets=dirt, forced=forced, max=amax, ties=ties)


def loss_terms(cls, box, dr, labels, tgt, dirt):
    """One frame, torch CPU float32 in the reference's expression order -> dict of the per-frame quantities (sums already
    normalised by max(npos, 1)) and the 16 metric counts."""
    cls = torch.as_tensor(cls).reshape(1, -1, 1)
    box = torch.as_tensor(box).reshape(1, -1, 7)
    dr = torch.as_tensor(dr).reshape(1, -1, 2)
    labels = torch.as_tensor(labels).reshape(1, -1)
    tgt = torch.as_tensor(tgt).reshape(1, -1, 7)
    dirt = torch.as_tensor(dirt).reshape(1, -1).long()
    pos = labels > 0
    npos = pos.sum(1, keepdim=True).float()
    norm = torch.clamp(npos, min=1.0)
    cls_w = ((labels == 0).float() + pos.float()) / norm
    reg_w = pos.float() / norm
    t = pos.float().unsqueeze(-1)
    ce = torch.clamp(cls, min=0) - cls * t + torch.log1p(torch.exp(-torch.abs(cls)))
    p = torch.sigmoid(cls)
    p_t = t * p + (1 - t) * (1 - p)
    focal = torch.pow(1.0 - p_t, 2.0) * (t * 0.25 + (1 - t) * 0.75) * ce * cls_w.unsqueeze(2)
    bp = torch.cat([box[..., :-1], torch.sin(box[..., -1:]) * torch.cos(tgt[..., -1:])], -1)
    bt = torch.cat([tgt[..., :-1], torch.cos(box[..., -1:]) * torch.sin(tgt[..., -1:])], -1)
    ad = torch.abs(bp - bt)
    lt = torch.le(ad, 1 / 9.0).type_as(ad)
    loc = (lt * 0.5 * torch.pow(ad * 3.0, 2) + (ad - 0.5 / 9.0) * (1.0 - lt)) * reg_w.unsqueeze(-1)
    dir_ce = torch.nn.functional.cross_entropy(dr.reshape(-1, 2), dirt.reshape(-1), reduction="none").reshape(1, -1)
    dirl = dir_ce * (pos.float() / torch.clamp(pos.float().sum(-1, keepdim=True), min=1.0))
    out = dict(npos=float(npos), loc=float(loc.sum()), cls_pos=float((pos.float() * focal.reshape(1, -1)).sum()),
               cls_neg=float(((labels == 0).float() * focal.reshape(1, -1)).sum()), dir=float(dirl.sum()))
    out["counts"] = metric_counts(labels, p.reshape(1, -1))
    return out


def metric_counts(labels, scores):
    """_calc_binary_metrics (metrics.py:55-69) with weights = labels != -1 -> int64[4 thresholds, (tp, tn, fp, fn)]."""
    labels = torch.as_tensor(labels).reshape(-1)
    scores = torch.as_tensor(scores).reshape(-1)
    w = labels != -1
    res = np.zeros((4, 4), np.int64)
    for i, th in enumerate(THRESHOLDS):
        pt = scores > th
        tr, fa = labels > 0, labels == 0
        res[i] = [int((w & tr & pt).sum()), int((w & fa & ~pt).sum()), int((w & fa & pt).sum()), int((w & tr & ~pt).sum())]
    return res


def batch_loss(frames):
    """The reference's six keys from per-frame loss_terms dicts (sums over frames / B, weights 0.25 / 1.0 / 0.2)."""
    B = len(frames)
    loc = sum(f["loc"] for f in frames) / B * 0.25
    cpos = sum(f["cls_pos"] for f in frames) / B
    cneg = sum(f["cls_neg"] for f in frames) / B
    cls = sum(f["cls_pos"] + f["cls_neg"] for f in frames) / B
    dirl = sum(f["dir"] for f in frames) / B
    return dict(loss=loc + cls + 0.2 * dirl, cls_pos_loss=cpos, cls_neg_loss=cneg, dir_loss=dirl, cls_loss=cls, loc_loss=loc)
