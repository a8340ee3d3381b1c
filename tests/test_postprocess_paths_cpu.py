"""Preconditions of tests/test_postprocess_paths_gpu.py, asserted on the CPU oracle alone: every case of
tests/postprocess_cases.py reaches the device path it is named after (more candidates than nms_pre_max, a sweep deeper than
the prefetched column tiles, a tie group across the K boundary, a short list that overflows, ...), and every rotated case
keeps the reference's IoUs at least 1e-4 from the threshold.  A case that stops meeting its precondition fails here, on a
machine without a GPU, instead of passing vacuously there."""
import numpy as np
import pytest

import postprocess_cases as P
from oracle import c_oracle as C
from oracle import pp_oracle as O

FAR = (P.NMS_AHEAD + 1) * 64  # first position in score order whose column tile is beyond the prefetched ones of row tile 0


# ------------------------------------------------------------------ plumbing
def test_oracle_keywords_at_defaults_change_nothing():
    logits, box, dr, mask = P.recipe_r(5)
    g = P.geometry()
    for mode, fn in (("aabb", C.nms_aabb), ("rotated", C.nms_rotated)):
        a = O.postprocess(logits, box, dr, mask, g["anchors"], g["class_masks"], g["center_limit"], mode, nms_fn=fn)
        b = O.postprocess(logits, box, dr, mask, g["anchors"], g["class_masks"], g["center_limit"], mode, nms_fn=fn,
                          pre_max=1000, post_max=300, iou_thr=0.1, score_thr=0.05)
        assert a[1] == b[1] and sum(a[1]) > 0
        assert a[0].tobytes() == b[0].tobytes()


def test_geometry_and_recipe():
    g = P.geometry()
    assert g["anchors"].shape == (P.A, 7)
    assert [tuple(v) for v in g["class_masks"].values()] == list(P.CLASS_RANGES)
    assert min(e - s for s, e in P.CLASS_RANGES) > P.SHORT_CAP
    logits, _, _, mask = P.recipe_r(5)
    assert np.unique(logits).size == P.A  # tie-free
    assert all(int(mask[s:e].sum()) > P.SHORT_CAP for s, e in P.CLASS_RANGES)


# ------------------------------------------------------------------ NMS-depth cases
@pytest.mark.parametrize("case", list(P.NMS_CASES))
def test_nms_case_reaches_its_depth(case):
    pre, post, iou, mode, seed = P.NMS_CASES[case]
    det, counts, info, margin = P.nms_reference(case)
    last = [P.last_emitted(i, post) for i in info]
    print(f"[pp paths] {case}: candidates {[i['n_cand'] for i in info]}, NMS survivors {[int(i['keep'].size) for i in info]}, "
          f"last emitted position / cut reached {last}, rows {counts}, smallest |IoU - thr| {margin:.3g}")
    assert all(i["n_cand"] > pre for i in info)  # every class fills all nms_pre_max rows
    assert all(i["idx"].size == pre for i in info)
    if mode == "rotated":
        # the band test_rotated_iou_and_nms allows between the device's and the reference's rotated IoU on non-degenerate pairs
        assert margin >= 1e-4, margin
    pos = [p for p, _ in last]
    cut = [c for _, c in last]
    if case.startswith("far-aabb"):  # all 19 tiles swept, the last tile has one column, the cut is never reached
        assert -(-pre // 64) == 19 and pre % 64 == 1
        assert all(1149 <= p <= 1152 for p in pos) and not any(cut)
    elif case.startswith("far-rot"):  # class 0 sweeps beyond the prefetched tiles, the other two reach the cut in tile 16
        assert pos[0] >= FAR and cut == [False, True, True] and all(1024 <= p < FAR for p in pos[1:])
    elif case == "max-aabb-s5":  # kept rows up to tile 44, the cut reached in the middle of the sweep
        assert pos == [2848, 1644, 1901] and all(cut)
    elif case.startswith("mid-rot"):
        assert all(cut) and all(700 <= p < FAR for p in pos) and counts == [700, 700, 700]
    elif case == "max-rot-s5":  # the cut falls on the first row of tile 16
        assert pos == [1025, 1025, 1025] and all(cut)
    elif case.startswith("tile-") and case.endswith("40"):  # one tile, post_max == pre_max
        assert pre == post == 40 and max(pos) == 39
    elif case.startswith("tile-"):  # post_max == 1
        assert post == 1 and pos == [0, 0, 0] and counts == [1, 1, 1]
    else:  # the defaults on this grid: 16 tiles, no far fold
        assert (pre, post, iou) == (1000, 300, 0.1) and max(pos) < FAR and not any(cut)
    if case.startswith(("far-", "max-aabb")):
        assert max(pos) >= FAR


def test_nms_cases_cover_the_far_fold_with_and_without_the_cut():
    far = {c: [P.last_emitted(i, P.NMS_CASES[c][1]) for i in P.nms_reference(c)[2]] for c in P.NMS_CASES if c.startswith(("far-", "max-aabb"))}
    flat = [x for v in far.values() for x in v]
    assert any(p >= FAR and not cut for p, cut in flat) and any(p >= FAR and cut for p, cut in flat)
    # a suppression through the far fold must matter: some row beyond the prefetched tiles is suppressed by a row kept more
    # than NMS_AHEAD tiles before it (otherwise a fold that does nothing would pass)
    for c in ("far-aabb-s5", "max-aabb-s5"):
        pre, post, iou, mode, seed = P.NMS_CASES[c]
        hit = 0
        for i in P.nms_reference(c)[2]:
            d, keep = i["dets"], i["keep"][:post]
            gone = np.setdiff1d(np.arange(FAR, int(keep[-1]) + 1), keep)
            for j in gone[:200]:
                early = keep[keep // 64 + P.NMS_AHEAD < j // 64]
                late = keep[(keep // 64 + P.NMS_AHEAD >= j // 64) & (keep < j)]
                sup = lambda rows: any(O.aabb_iou_plus1(d[r, :4], d[j, :4]) > np.float32(iou) for r in rows)
                hit += bool(early.size and sup(early) and not sup(late))
        print(f"[pp paths] {c}: {hit} rows suppressed through the far-tile fold only")
        assert hit > 0


# ------------------------------------------------------------------ selection cases
def test_boundary_logits():
    hi, lo, margin = P.boundary_pair(0.05)
    assert (int(hi.view(np.uint32)), int(lo.view(np.uint32))) == (0xC03C71B0, 0xC03C71B1)
    assert int(O.sigmoid_f32(hi).view(np.uint32)) == 0x3D4CCCCD == int(np.float32(0.05).view(np.uint32))
    assert int(O.sigmoid_f32(lo).view(np.uint32)) == 0x3D4CCCCA
    for thr in sorted({t for _, t in P.SELECT_PARAMS}):
        hi, lo, margin = P.boundary_pair(thr)
        print(f"[pp paths] threshold {thr}: hi {int(hi.view(np.uint32)):#x} lo {int(lo.view(np.uint32)):#x} midpoint margin {margin:.3g}"
              f"{'' if P.s4_usable(thr) else ' (S4 dropped)'}")
        assert O.sigmoid_f32(hi) >= np.float32(thr) > O.sigmoid_f32(lo) and lo < hi
        if P.s4_usable(thr):
            assert margin >= 1e-9
    assert P.s4_usable(0.05)  # the reference's own operating point must keep its equality probe


def _paths(case, K, thr):
    logits, mask = P.select_inputs(case, K, thr)
    return [P.predicted_path(logits, mask, c, K, thr) for c in range(3)]


@pytest.mark.parametrize("K,thr", P.SELECT_PARAMS)
def test_selection_cases_reach_their_paths(K, thr):
    ref = {c: P.select_reference(c, K, thr) for c in P.SELECT_CASES}
    paths = {c: _paths(c, K, thr) for c in P.SELECT_CASES if ref[c] is not None}
    for c, p in paths.items():
        print(f"[pp paths] K {K} thr {thr} {c}: " + ", ".join(f"{q['total']} cand -> {q['path']} ({q['short']} keys{', direct append' if q['direct'] else ''})"
                                                             for q in p))
        assert [q["total"] for q in p] == [r["n_cand"] for r in ref[c]]
        assert [r["idx"].size for r in ref[c]] == [min(q["total"], K) for q in p]
    live = thr <= 0.5  # the recipes' scores end at sigmoid(4) = 0.982: at 0.999 only S3 and S6 have candidates
    logits, mask = P.select_inputs("S1-ties", K, thr)
    if live:
        # S1: the tie group of the K-th score straddles K, so the order inside it decides the result
        for c, (s, e) in enumerate(P.CLASS_RANGES):
            r = ref["S1-ties"][c]
            sc = O.sigmoid_f32(logits[s:e][mask[s:e]])
            kth = r["score"][K - 1]
            assert (sc > kth).sum() < K < (sc >= kth).sum()
            grp = r["idx"][r["score"] == kth]
            assert (np.diff(grp) > 0).all()  # lower anchor id first
        # S2: the K lowest masked-in anchor ids of each class, through the radix fallback and the direct append
        for c, (s, e) in enumerate(P.CLASS_RANGES):
            r = ref["S2-all-equal"][c]
            assert np.array_equal(r["idx"], (np.nonzero(mask[s:e])[0] + s)[:K]) and (r["score"] == np.float32(0.5)).all()
        assert all(q["path"] == "radix" and q["direct"] for q in paths["S2-all-equal"])
        assert any(q["path"] == "radix" for q in paths["S5-one-bin"])
        l5, _ = P.select_inputs("S5-one-bin", K, thr)
        for c, (s, e) in enumerate(P.CLASS_RANGES):  # thousands of distinct scores in at most two coarse bins
            sc = O.sigmoid_f32(l5[s:e])
            sc = sc[sc >= np.float32(thr)]
            bins = (sc.view(np.uint32).astype(np.int64) - int(np.float32(thr).view(np.uint32))) >> P.shift_for(thr)
            assert np.unique(bins).size <= 2 and np.unique(sc).size >= 3000
    else:
        assert all(q["path"] == "none" for c in ("S1-ties", "S2-all-equal", "S5-one-bin") for q in paths[c])
    if K == P.SHORT_CAP:  # no slack in the short list: the radix path is the normal path whenever total > K
        assert all(q["path"] == "radix" for c in ("S1-ties", "S2-all-equal", "S5-one-bin", "S6-saturated") for q in paths[c])
    # S3: the "take everything" branch and its edges
    a, b = paths["S3-counts-a"], paths["S3-counts-b"]
    assert [q["total"] for q in a] == [0, K - 1, K + 1] and [q["total"] for q in b] == [K, 1, K]
    assert [q["path"] for q in a] == ["none", "all", "short"] and [q["path"] for q in b] == ["all", "all", "all"]
    for c in ("S3-counts-a", "S3-counts-b"):
        for r in ref[c]:
            assert np.unique(r["score"]).size == r["score"].size  # distinct passing values
    # S4: 300 masked-in anchors per class exactly at the threshold pass, 300 one float below fail
    if ref["S4-boundary"] is not None:
        hi, lo, _ = P.boundary_pair(thr)
        l4, m4 = P.select_inputs("S4-boundary", K, thr)
        for c, (s, e) in enumerate(P.CLASS_RANGES):
            assert int(((l4[s:e] == hi) & m4[s:e]).sum()) == 300 == int(((l4[s:e] == lo) & m4[s:e]).sum())
            r = ref["S4-boundary"][c]
            assert r["n_cand"] == 300 and r["idx"].size == min(300, K) and (r["score"] == np.float32(thr)).all()
    else:
        assert thr != 0.05
    # S6: ties in the top bin, more of them than the short list holds
    for c, (s, e) in enumerate(P.CLASS_RANGES):
        r = ref["S6-saturated"][c]
        assert (r["score"] == np.float32(1.0)).all() and r["idx"].size == K and (np.diff(r["idx"]) > 0).all()
    assert all(q["path"] == "radix" for q in paths["S6-saturated"])
