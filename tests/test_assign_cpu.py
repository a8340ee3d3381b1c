"""CPU (-m "not gpu"): the numpy / torch restatements of the reference's training-target side (tests/assign_ref.py) reproduce the
goldens made by running the reference itself (tests/golden/make_assign_goldens.py), and the labels do not depend on how numba
would type iou_jit.

Typing: the goldens come from iou_jit run as plain Python, every intermediate float32 -- what the GPU kernels compute.  Real numba
types `+ eps` (a float64 argument) as double, so iw, ih, the areas and the quotient run in fp64 and only the store rounds.  The
typing test runs the restatement both ways on every golden frame and requires identical labels, forced sets and targets."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, golden, load_pkg
import assign_ref

sys.path.insert(0, GOLDEN)


def setup():
    eng = load_pkg("engine")
    synth = load_pkg("synth")
    cfg = synth.load_config("eight_20cm")
    vs, off, grid, rd, _ = eng.snap_geometry(cfg)
    anchors, bv, _, cm = eng.build_anchor_tables(off, rd, grid, vs)
    t = eng.CLASS_TABLE
    names = list(cm)
    return anchors, bv, list(cm.values()), [t[n]["matched_threshold"] for n in names], [t[n]["unmatched_threshold"] for n in names]


def golden_frame(g, f, A):
    mask = np.unpackbits(g[f"mask_{f}"])[:A].astype(bool)
    labels = g[f"labels_{f}"].astype(np.int32)
    tgt = np.zeros((A, 7), np.float32)
    tgt[g[f"pos_{f}"]] = g[f"pos_targets_{f}"]
    dirt = np.unpackbits(g[f"dir_{f}"])[:A].astype(np.int32)
    return mask, g[f"gt_{f}"], g[f"gt_cls_{f}"], labels, tgt, dirt


@pytest.fixture(scope="module")
def geo():
    return setup()


@pytest.fixture(scope="module")
def gold():
    return golden("assign_eight_20cm")


def test_restated_assign_matches_reference_goldens(geo, gold):
    anchors, bv, ranges, tm, tu = geo
    A = anchors.shape[0]
    assert [list(r) for r in gold["class_ranges"]] == [list(r) for r in ranges]
    for f in range(int(gold["nframes"])):
        mask, gt, gc, labels, tgt, dirt = golden_frame(gold, f, A)
        r = assign_ref.assign_frame(anchors, bv, ranges, tm, tu, gt, gc, mask)
        assert np.array_equal(r["labels"], labels), f"frame {f}"
        assert np.array_equal(r["bbox_targets"], tgt), f"frame {f}"
        assert np.array_equal(r["dir_targets"], dirt), f"frame {f}"
        assert float(r["outside_w"].sum()) == float(gold[f"ow_sum_{f}"])


def test_golden_covers_the_edge_cases(geo, gold):
    anchors, bv, ranges, tm, tu = geo
    A = anchors.shape[0]
    m0, gt0, gc0, *_ = golden_frame(gold, 0, A)
    assert set(gc0.tolist()) == {1, 2, 3}
    q = np.float32(np.pi / 4)
    assert (gt0[:, 6] == q).any() and (gt0[:, 6] == -q).any()
    assert (np.abs(gt0[:, 6]) > q).any() and (np.abs(gt0[:, 6]) < q).any()
    assert assign_ref.assign_frame(anchors, bv, ranges, tm, tu, gt0, gc0, m0)["ties"] > 0
    assert len(gold["gt_1"]) == 0
    assert not np.unpackbits(gold["mask_2"])[:A].any() and np.unpackbits(gold["mask_3"])[:A].all()
    assert not (gold["gt_cls_3"] == 3).any()
    rb, rk = gold["range_boxes"], gold["range_keep"]
    assert rk.any() and not rk.all() and (rb[:, 6] > 0).any() and (rb[:, 6] < 0).any()


def test_restated_loss_matches_reference(geo, gold):
    import make_assign_goldens as mk
    anchors, *_ = geo
    A = anchors.shape[0]
    lg = golden("loss_eight_20cm")
    frames = [int(f) for f in lg["frames"]]
    cls, box, dr = mk.logits(int(lg["seed"]), A, len(frames))
    from make_goldens import sha
    assert sha(cls, box, dr) == str(lg["logits_sha"])
    per = []
    counts = np.zeros((4, 4), np.int64)
    for i, f in enumerate(frames):
        _, _, _, labels, tgt, dirt = golden_frame(gold, f, A)
        t = assign_ref.loss_terms(cls[i], box[i], dr[i], labels, tgt, dirt)
        per.append(t)
        counts += t["counts"]
    got = assign_ref.batch_loss(per)
    for k, v in zip(lg["keys"], lg["values"]):
        assert got[str(k)] == pytest.approx(float(v), rel=1e-5), k
    assert np.array_equal(counts, lg["counts"])


def test_combine_terms_matches_restatement(geo, gold):
    """framework.loss_generator.combine_terms on per-frame terms laid out as pp_target_loss writes them."""
    lgm = load_pkg("framework.loss_generator")
    frames = [dict(npos=3, loc=0.5, cls_pos=0.25, cls_neg=2.0, dir=0.7), dict(npos=0, loc=0.0, cls_pos=0.0, cls_neg=1.5, dir=0.0)]
    terms = np.zeros((2, 21))
    for i, f in enumerate(frames):
        terms[i, :5] = [f["npos"], f["loc"], f["cls_pos"], f["cls_neg"], f["dir"]]
    a, b = lgm.combine_terms(terms), assign_ref.batch_loss(frames)
    assert set(a) == set(b) and all(a[k] == pytest.approx(b[k], rel=1e-12) for k in a)


def test_numba_typing_does_not_change_the_golden_assignment(geo, gold):
    anchors, bv, ranges, tm, tu = geo
    A = anchors.shape[0]
    thr = sorted(set(np.float32(v) for v in tm + tu))
    margin, ties32, ties64 = np.inf, 0, 0
    for f in range(int(gold["nframes"])):
        mask, gt, gc, *_ = golden_frame(gold, f, A)
        r32 = assign_ref.assign_frame(anchors, bv, ranges, tm, tu, gt, gc, mask, typing="f32")
        r64 = assign_ref.assign_frame(anchors, bv, ranges, tm, tu, gt, gc, mask, typing="f64")
        assert np.array_equal(r32["labels"], r64["labels"]), f"frame {f}"
        assert np.array_equal(r32["forced"], r64["forced"]), f"frame {f}"
        assert np.array_equal(r32["bbox_targets"], r64["bbox_targets"]), f"frame {f}"
        mx = r32["max"][~np.isnan(r32["max"])]
        if mx.size:
            margin = min(margin, float(np.min(np.abs(mx[:, None].astype(np.float64) - np.array(thr, np.float64)[None, :]))))
        ties32 += r32["ties"]
        ties64 += r64["ties"]
    print(f"\nsmallest |max - threshold| {margin:.3e}; ties at box maxima f32 {ties32}, f64 {ties64}")
    assert ties32 == ties64


def test_gt_range_filter_matches_reference(gold):
    kio = load_pkg("kitti_io")
    eng = load_pkg("engine")
    dr = eng.snap_geometry(load_pkg("synth").load_config("eight_20cm"))[4]
    # the golden's boxes straddle, touch and just miss every edge and corner of the range, at rotations of both signs
    assert np.array_equal(kio.gt_in_range(gold["range_boxes"], dr[[0, 1, 3, 4]]), gold["range_keep"])
    gt = gold["range_boxes"]
    cls_ids = (np.arange(len(gt)) % 3 + 1).astype(np.int32)
    names = np.array(["vehicle", "pedestrian", "cyclist", "cone"])[cls_ids - 1]
    names[0] = "cone"
    annos = dict(name=names, location=gt[:, :3], dimensions=gt[:, 3:6], rotation_y=gt[:, 6] + np.float32(2 * np.pi))
    cls, boxes = kio.gt_from_annos(annos, ["vehicle", "pedestrian", "cyclist"], dr)
    keep = gold["range_keep"].copy()
    keep[0] = False
    assert np.array_equal(cls, cls_ids[keep])
    assert np.allclose(boxes[:, 6], gt[keep, 6], atol=1e-5) and np.all(np.abs(boxes[:, 6]) <= np.pi + 1e-6)


def test_label_order_follows_reference_when_matched_is_below_unmatched(geo):
    """anchor_assigner.py:381-392 sets pos (>= matched), then bg (< unmatched) overwrites it, then forced: with matched < unmatched
    an anchor between the two thresholds is background, not positive."""
    anchors, bv, ranges, tm, tu = geo
    s, e = ranges[1]
    gt = np.array([[10.2, -20.2, -1.0, 1.4, 1.4, 1.7, 0.0]], np.float32)
    mask = np.zeros(anchors.shape[0], bool)
    mask[s:e] = True
    r = assign_ref.assign_frame(anchors, bv, ranges, [0.6, 0.05, 0.5], [0.45, 0.3, 0.25], gt, [2], mask)
    mid = (r["max"] >= 0.05) & (r["max"] < 0.3) & ~r["forced"]
    assert mid.any() and (r["labels"][mid] == 0).all()
