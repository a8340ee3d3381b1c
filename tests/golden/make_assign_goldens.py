#!/usr/bin/env python3
"""Generate tests/golden/assign_eight_20cm.npz and loss_eight_20cm.npz by RUNNING THE REFERENCE (needs the reference tree; ~1 min).

    python tests/golden/make_assign_goldens.py

Reuses make_goldens.install_shims (numba as identity decorators, so iou_jit runs as the plain Python it is written in: under
numpy >= 2 every intermediate stays float32) and its helpers.  Runs the reference's own AnchorAssigner(cfg).assign,
LossGenerator(cfg).generate (torch, CPU), metrics._calc_binary_metrics (Metric.update's counts; Metric itself allocates on CUDA)
and box_np_ops.filter_gt_box_outside_range on the eight_20cm geometry, the one whose hard-coded 400 x 400 feature map equals ours.

Frames (the generator asserts the cases exist):
  0  mask from the synthetic cloud seed 1000 (reference voxeliser + create_mask(gpu=False)); boxes of all three classes on
     occupied ground, rotations on both sides of +-pi/4 and exactly at +-pi/4 (float32); a box out of range (matches no
     anchor: gmax = -1); a 3 x 3 m pedestrian box that contains whole anchors (exact ties at its maximum)
  1  the same mask, no boxes
  2  all-zero mask, boxes
  3  all-ones mask, vehicle and pedestrian boxes only (cyclist: a class with no boxes)
Storage: masks and dir targets bit-packed, labels int8, bbox targets only for the positive rows.  The loss fixture's logits come
from numpy.random.default_rng(seed); only the seed and a sha256 of the arrays are stored.
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import REF, ROOT, install_shims, save, sha  # noqa: E402

CLOUD_SEED = 1000
LOGIT_SEED = 20260
LOSS_FRAMES = (0, 3)
SCORE_MARGIN = 1e-6  # no sigmoid(cls) of the loss fixture lies this close to a metric threshold


def logits(seed, A, nb):
    rng = np.random.default_rng(seed)
    cls = (rng.standard_normal((nb, A, 1)) * 2.0 - 3.0).astype(np.float32)
    box = (rng.standard_normal((nb, A, 7)) * 0.3).astype(np.float32)
    dr = rng.standard_normal((nb, A, 2)).astype(np.float32)
    # keep every score clear of the metric thresholds, so that no sigmoid implementation's last-ulp rounding decides a count
    for t in (0.1, 0.3, 0.5, 0.7):
        near = np.abs(1.0 / (1.0 + np.exp(-cls.astype(np.float64))) - t) <= SCORE_MARGIN
        cls[near] += np.float32(0.01)
    return cls, box, dr


def frame_boxes(rng, pts):
    """Boxes on occupied ground of the cloud: (x, y, z, l, w, h, r) float32 and 1-based class ids."""
    sizes = {1: (4.5, 1.9, 1.6), 2: (0.8, 0.7, 1.75), 3: (1.8, 0.7, 1.7)}
    q = np.float32(np.pi / 4)
    rots = [0.0, q, -q, np.float32(0.7), np.float32(0.9), np.float32(-0.8), np.float32(1.57), np.float32(2.5), np.float32(-3.0)]
    near = pts[(np.abs(pts[:, 0]) < 50) & (np.abs(pts[:, 1]) < 50)]
    boxes, cls = [], []
    for i in range(18):
        c = 1 + i % 3
        p = near[int(rng.integers(0, near.shape[0]))]
        s = sizes[c]
        boxes.append([p[0], p[1], -1.0, s[0] * rng.uniform(0.9, 1.1), s[1] * rng.uniform(0.9, 1.1), s[2], rots[i % len(rots)]])
        cls.append(c)
    boxes.append([150.0, 150.0, -1.0, 4.5, 1.9, 1.6, 0.0])  # beyond the range: overlaps no anchor
    cls.append(1)
    boxes.append([10.2, -20.2, -1.0, 3.0, 3.0, 1.7, 0.0])  # holds whole pedestrian anchors: ties at the box maximum
    cls.append(2)
    return np.array(boxes, np.float32), np.array(cls, np.int32)


def range_edge_boxes(det_range):
    """Frame 0's kind of boxes plus edge cases of the range filter: centres on, inside and outside each edge and corner;
    l = 4, w = 2, so at r = 0 a centre l/2 beyond an x edge puts two corners exactly on it (strictly outside)."""
    x0, y0, x1, y1 = (float(v) for v in np.asarray(det_range)[[0, 1, 3, 4]])
    rows = []
    rots = [0.0, 0.3, -0.3, np.pi / 2, -np.pi / 2, np.pi / 4, -2.0, 3.0]
    for cx, cy in [(x1, 0.0), (x0, 5.0), (10.0, y1), (-7.0, y0), (x1, y1), (x0, y0), (x1, y0), (x0, y1)]:
        sx = np.sign(cx) if abs(cx) in (abs(x0), abs(x1)) else 0.0
        sy = np.sign(cy) if abs(cy) in (abs(y0), abs(y1)) else 0.0
        for d in (-1.5, -0.5, 0.0, 0.99, 1.0, 1.01, 2.0, 2.2):
            for r in rots[:4] if d not in (1.0, 2.0) else rots:
                rows.append([cx + sx * d, cy + sy * d, -1.0, 4.0, 2.0, 1.6, r])
    return np.array(rows, np.float32)


def main():
    install_shims()
    sys.path.insert(0, REF)
    sys.path.insert(0, ROOT)
    import importlib
    import torch
    torch.set_num_threads(8)
    synth = importlib.import_module("3d_object_detection_amd.synth")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import assign_ref
    from framework.voxel_generator import VoxelGenerator
    from framework.anchor_assigner import AnchorAssigner
    from framework.loss_generator import LossGenerator
    from framework.metrics import _calc_binary_metrics
    from framework import box_np_ops

    cfg = synth.load_config("eight_20cm")
    vg = VoxelGenerator(cfg)
    aa = AnchorAssigner(cfg)
    A = aa.anchors.shape[0]
    pts = synth.lidar_cloud("eight_20cm", seed=CLOUD_SEED)
    _, c, _ = vg.generate(pts)
    real = aa.create_mask(c, cfg["grid_size"], vg.voxel_size, vg.offset, gpu=False).astype(bool)
    rng = np.random.default_rng(5)
    b0, c0 = frame_boxes(rng, pts)
    b2, c2 = frame_boxes(rng, pts)
    b3, c3 = frame_boxes(rng, pts)
    keep3 = c3 != 3
    frames = [(real, b0, c0), (real, np.zeros((0, 7), np.float32), np.zeros(0, np.int32)), (np.zeros(A, bool), b2, c2),
              (np.ones(A, bool), b3[keep3], c3[keep3])]
    names = list(aa.class_masks.keys())
    ranges = list(aa.class_masks.values())
    thr_m = [float(aa.matched_threshold[s]) for s, _ in ranges]
    thr_u = [float(aa.unmatched_threshold[s]) for s, _ in ranges]
    out = dict(class_names=np.array(names), class_ranges=np.array(ranges, np.int32), cloud_seed=CLOUD_SEED, nframes=len(frames),
               anchors_sha=sha(aa.anchors))
    results = []
    for f, (m, b, cl) in enumerate(frames):
        lab, tgt, ow, dirt = aa.assign(cl, b, m)
        assert lab.dtype == np.int32 and tgt.dtype == np.float32 and ow.dtype == np.float32 and dirt.dtype == np.int32
        assert lab.shape == (A,) and tgt.shape == (A, 7)
        r = assign_ref.assign_frame(aa.anchors, aa.anchors_bv, ranges, thr_m, thr_u, b, cl, m)
        assert np.array_equal(r["labels"], lab) and np.array_equal(r["bbox_targets"], tgt) and np.array_equal(r["dir_targets"], dirt)
        pos = np.nonzero(lab > 0)[0].astype(np.int32)
        out.update({f"mask_{f}": np.packbits(m), f"gt_{f}": b, f"gt_cls_{f}": cl, f"labels_{f}": lab.astype(np.int8),
                    f"pos_{f}": pos, f"pos_targets_{f}": tgt[pos], f"dir_{f}": np.packbits(dirt.astype(bool)),
                    f"ow_sum_{f}": float(ow.sum())})
        results.append((lab, tgt, dirt, r))
        print(f"frame {f}: {len(b)} boxes, {int(m.sum())} inside, {len(pos)} positive, {r['ties']} ties")
    # the cases the tests rely on
    assert results[0][3]["ties"] > 0, "no exact tie at a box maximum"
    ov = assign_ref.iou(aa.anchors_bv[real], assign_ref.near_bv(b0[-2:-1]))
    assert ov.max() == 0, "the out-of-range box overlaps an anchor"
    assert len(frames[1][1]) == 0 and not frames[2][0].any() and frames[3][0].all() and not (frames[3][2] == 3).any()
    assert set(c0.tolist()) == {1, 2, 3}
    q = np.float32(np.pi / 4)
    assert (b0[:, 6] == q).any() and (b0[:, 6] == -q).any()

    # filter_gt_box_outside_range (box_np_ops.py:6-16), for kitti_io.gt_from_annos: frame 0's boxes plus boxes that straddle,
    # touch or just miss every edge and corner of the range, at several rotations of both signs
    rb = range_edge_boxes(vg.detection_range)
    keep = np.asarray(box_np_ops.filter_gt_box_outside_range(rb, vg.detection_range[[0, 1, 3, 4]]), bool)
    assert keep.any() and not keep.all()
    out["range_boxes"] = rb
    out["range_keep"] = keep
    save("assign_eight_20cm", **out)

    # ---------------- loss + metric counts (LOSS_FRAMES as one batch) ----------------
    nb = len(LOSS_FRAMES)
    cls, box, dr = logits(LOGIT_SEED, A, nb)
    sc = 1.0 / (1.0 + np.exp(-cls.astype(np.float64)))
    margin = min(float(np.abs(sc - t).min()) for t in assign_ref.THRESHOLDS)
    assert margin > SCORE_MARGIN, f"logit seed {LOGIT_SEED}: a score lies {margin:.2e} from a metric threshold"
    lab = np.stack([results[f][0] for f in LOSS_FRAMES])
    tgt = np.stack([results[f][1] for f in LOSS_FRAMES])
    dirt = np.stack([results[f][2] for f in LOSS_FRAMES])
    lg = LossGenerator({"box_code_size": 7, "device": torch.device("cpu")})
    preds = {"cls_preds": torch.from_numpy(cls), "box_preds": torch.from_numpy(box), "dir_preds": torch.from_numpy(dr)}
    ret = lg.generate(preds, {"labels": lab, "bbox_targets": tgt, "dir_targets": dirt})
    scores = torch.max(torch.sigmoid(torch.from_numpy(cls)), dim=-1)[0]
    lt = torch.from_numpy(lab)
    counts = np.array([[float(v) for v in _calc_binary_metrics(lt, scores, (lt != -1).float(), th)] for th in assign_ref.THRESHOLDS])
    save("loss_eight_20cm", seed=LOGIT_SEED, frames=np.array(LOSS_FRAMES, np.int32), logits_sha=sha(cls, box, dr), score_margin=margin,
         keys=np.array(list(ret.keys())), values=np.array([float(v) for v in ret.values()], np.float64), counts=counts.astype(np.int64))
    print({k: float(v) for k, v in ret.items()}, "margin", margin)


if __name__ == "__main__":
    main()
