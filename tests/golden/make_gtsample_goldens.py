#!/usr/bin/env python3
"""Generate tests/golden/gtsample_small.npz by RUNNING THE REFERENCE (needs the reference tree; a few seconds).

    python tests/golden/make_gtsample_goldens.py

Reuses make_goldens.install_shims (numba as identity decorators) and runs the reference's three primitives of ground-truth sampling
on small synthetic frames:
  box_np_ops.points_in_rbbox                       membership tables, and both counts of create_info.py:172-183 (num_points: the
                                                   boxes as they are; difficulty: (l, w, h) + (1.2, 0.5, 8)); create_info.py itself
                                                   cannot be imported (skimage), so its two statements are repeated here
  augmentation.box_collision_test on box_np_ops.center_to_corner_box2d corners     collision matrices candidate x (existing + candidate)
  augmentation.remove_points_in_boxes              the cloud after removal

Frame 0 is the count / extract frame of tests/test_gtsample_gpu.py: 3000 points and seven boxes -- two overlapping boxes sharing
points, a box with 0 points, one with exactly 1, one with 65 (a wave boundary), one with about 700 spread over the cloud, and one
whose members are the cloud's first and last point.  Frame 1 has 0 points and two boxes, frame 2 has 500 points and no box.

The generator asserts:
  - every point-face sign (both box sizes) and every collision comparison lies at least MARGIN from its threshold on the numpy
    restatement (tests/gtsample_ref.py); points that violate it are trimmed from the inputs before anything is computed;
  - the restatement reproduces every table, count, matrix and cloud of the reference;
  - no collision decision rests on box_collision_test's containment branch, which numba runs and plain Python does not (the nested
    case is tested on the GPU against the restatement);
  - the cases above exist.
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import REF, ROOT, install_shims, save  # noqa: E402

MARGIN = 2e-5  # as make_augment_goldens.py measured it
EXTRA = np.array([1.2, 0.5, 8])  # create_info.py:180

BOXES0 = np.array([[10.0, 5.0, -1.0, 4.5, 1.9, 1.6, 0.3],      # 0, 1: overlapping, sharing points
                   [11.5, 5.3, -1.0, 4.5, 1.9, 1.6, 0.35],
                   [-30.0, -30.0, -1.0, 4.2, 1.8, 1.5, 1.1],   # 2: no point
                   [-30.0, 30.0, -1.0, 0.8, 0.7, 1.75, -0.7],  # 3: one point
                   [30.0, -30.0, -1.0, 4.6, 2.0, 1.7, 2.9],    # 4: 65 points
                   [0.0, -20.0, -1.0, 20.0, 10.0, 4.0, 0.2],   # 5: about 700 points all over the cloud's order
                   [-10.0, 35.0, -1.0, 2.0, 2.0, 2.0, 0.5]],   # 6: the first and the last point
                  np.float32)
BOXES1 = np.array([[5.0, 5.0, -1.0, 4.0, 1.8, 1.5, 0.0], [-5.0, 8.0, -1.0, 0.8, 0.6, 1.7, 1.0]], np.float32)
N0, N2 = 3000, 500


def inside(rng, b, n, u=0.4):
    q = rng.uniform(-u, u, size=(n, 3))
    c, s = np.cos(b[6]), np.sin(b[6])
    lx, ly, lz = q[:, 0] * b[3], q[:, 1] * b[4], q[:, 2] * b[5]
    return np.stack([lx * c - ly * s + b[0], lx * s + ly * c + b[1], lz + b[2], rng.uniform(0, 1, n)], axis=1).astype(np.float32)


def near_plane(S, pts, boxes):
    """points within 2 MARGIN of a face plane of some box at either size"""
    near = np.zeros(pts.shape[0], bool)
    for extra in ((0, 0, 0), S.DIFFICULTY_EXTRA):
        for b in S.grown(boxes, extra):
            near |= (np.abs(S.signs(pts, b)) <= 2 * MARGIN).any(axis=1)
    return near


def frame0(S):
    rng = np.random.default_rng(400)
    b = BOXES0

    def clear(b_, n, u=0.4):  # n points inside b_, none within the margin of a plane of any box
        q = inside(rng, b_, 2 * n + 8, u)
        q = q[~near_plane(S, q, b)]
        assert q.shape[0] >= n
        return q[:n]

    special = np.concatenate([clear(b[0], 60, 0.6), clear(b[1], 60, 0.6), clear(b[3], 1), clear(b[4], 65), clear(b[5], 700, 0.45)])
    ends = clear(b[6], 2)
    fill = np.concatenate([rng.uniform(-40, 40, (2600, 2)), rng.uniform(-3, 1, (2600, 1)), rng.uniform(0, 1, (2600, 1))], axis=1).astype(np.float32)
    # no filler point in or near the boxes whose counts are the case
    fill = fill[~S.member_table(fill, b[[2, 3, 4, 5, 6]], (0.6, 0.6, 0.6)).any(axis=1)]
    fill = fill[~near_plane(S, fill, b)]
    mid = np.concatenate([special, fill])[:N0 - 2]
    assert mid.shape[0] == N0 - 2, "not enough filler points left after the trim"
    mid = mid[rng.permutation(mid.shape[0])]
    return np.ascontiguousarray(np.concatenate([ends[:1], mid, ends[1:]]).astype(np.float32))


SEL_EXIST = np.array([[10.0, 0.0, -1.0, 4.5, 1.9, 1.6, 0.2], [-10.0, 0.0, -1.0, 4.5, 1.9, 1.6, -0.4]], np.float32)  # row 1 plays the invalid box
SEL_CAND = np.array([[-9.0, 1.0, -1.0, 4.4, 1.8, 1.5, 0.9],     # 0: crosses existing 1 (the invalid one)         -> rejected
                     [20.0, 20.0, -1.0, 4.5, 1.9, 1.6, 0.1],    # 1: free                                          -> accepted
                     [21.5, 20.6, -1.0, 4.5, 1.9, 1.6, 0.7],    # 2: crosses candidate 1 (accepted)               -> rejected
                     [25.0, 22.0, -1.0, 4.5, 1.9, 1.6, 0.3],    # 3: crosses candidate 2 only (rejected)          -> accepted
                     [-25.0, 12.0, -1.0, 0.8, 0.7, 1.7, 1.3]],  # 4: free                                          -> accepted
                    np.float32)


def main():
    install_shims()
    sys.path.insert(0, REF)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gtsample_ref as S
    from framework import augmentation as ragm
    from framework import box_np_ops

    out = dict(margin=MARGIN, extra=EXTRA.astype(np.float32))
    rng = np.random.default_rng(401)
    p2 = np.concatenate([rng.uniform(-40, 40, (N2, 2)), rng.uniform(-3, 1, (N2, 1)), rng.uniform(0, 1, (N2, 1))], axis=1).astype(np.float32)
    frames = [(frame0(S), BOXES0), (np.zeros((0, 4), np.float32), BOXES1), (p2, np.zeros((0, 7), np.float32))]
    for f, (pts, boxes) in enumerate(frames):
        # create_info.py:172-183 on float32 lidar boxes
        if boxes.shape[0]:
            table = np.asarray(box_np_ops.points_in_rbbox(pts, boxes.copy()), bool).reshape(pts.shape[0], boxes.shape[0])
            big = boxes.copy()
            big[:, 3:6] = big[:, 3:6] + EXTRA
            table_d = np.asarray(box_np_ops.points_in_rbbox(pts, big), bool).reshape(pts.shape[0], boxes.shape[0])
        else:
            table = table_d = np.zeros((pts.shape[0], 0), bool)
        num, diff = table.sum(axis=0).astype(np.int32), table_d.sum(axis=0).astype(np.int32)
        margins = []
        assert np.array_equal(S.member_table(pts, boxes, margins=margins), table), f"frame {f}: membership differs from the reference"
        assert np.array_equal(S.member_table(pts, boxes, S.DIFFICULTY_EXTRA, margins), table_d), f"frame {f}: grown membership differs"
        assert np.array_equal(S.count(pts, boxes), num) and np.array_equal(S.count(pts, boxes, S.DIFFICULTY_EXTRA), diff)
        mmin = min(margins) if margins else np.inf
        assert mmin > MARGIN, f"frame {f}: a point-face sign lies {mmin:.2e} from zero"
        out.update({f"points_{f}": pts, f"boxes_{f}": boxes, f"table_{f}": table, f"num_points_{f}": num, f"difficulty_{f}": diff})
        print(f"frame {f}: {pts.shape[0]} points, {boxes.shape[0]} boxes, num_points {num.tolist()}, difficulty {diff.tolist()}, margin {mmin:.2e}")
    t0 = out["table_0"]
    n0 = out["num_points_0"]
    assert out["points_0"].shape[0] == N0 and (t0[:, 0] & t0[:, 1]).sum() > 0, "no point shared by the overlapping boxes"
    assert n0[2] == 0 and n0[3] == 1 and n0[4] == 65 and 600 <= n0[5] <= 800, n0
    m5 = np.nonzero(t0[:, 5])[0]
    assert len({int(i) // 256 for i in m5}) >= 10, "the large box's members do not spread over the cloud"
    assert np.nonzero(t0[:, 6])[0].tolist() == [0, N0 - 1], "box 6 must hold the first and the last point only"

    # collision matrices: the candidate as `boxes`, existing + candidates as `qboxes`
    allb = np.concatenate([SEL_EXIST, SEL_CAND])
    cc = box_np_ops.center_to_corner_box2d(SEL_CAND[:, :2], SEL_CAND[:, 3:5], SEL_CAND[:, 6])
    ca = box_np_ops.center_to_corner_box2d(allb[:, :2], allb[:, 3:5], allb[:, 6])
    coll = np.asarray(ragm.box_collision_test(cc, ca), bool)
    margins, contained = [], []
    mine = S.collision_matrix(SEL_CAND, allb, True)
    ne = SEL_EXIST.shape[0]
    off_diag = ~np.eye(len(SEL_CAND), len(allb), ne, dtype=bool)  # a box against itself is not a decision of the sampler
    assert np.array_equal(mine[off_diag], coll[off_diag]), "collision matrix differs from the reference"
    acc = S.select(SEL_EXIST, SEL_CAND, True, margins, contained)
    assert np.array_equal(acc, S.select(SEL_EXIST, SEL_CAND, False)), "a decision rests on the containment branch"
    pairs = [(i, k) for i in range(len(SEL_CAND)) for k in range(len(allb)) if k != ne + i]
    contained_pairs = [p for p in pairs if not coll[p] and S.collision_matrix(SEL_CAND[p[0]:p[0] + 1], allb[p[1]:p[1] + 1], True, margins)[0, 0]]
    assert not contained_pairs, f"containment decides {contained_pairs}"
    assert min(margins) > MARGIN, f"a collision comparison lies {min(margins):.2e} from its threshold"
    assert acc.tolist() == [False, True, False, True, True], acc
    assert coll[0, 1] and not coll[0, 0] and coll[2, ne + 1] and coll[3, ne + 2] and not coll[3, ne + 1] and not coll[3, :ne].any()
    out.update(sel_existing=SEL_EXIST, sel_cand=SEL_CAND, sel_collision=coll, sel_accept=acc, sel_margin=min(margins))
    print(f"select: accept {acc.tolist()}, margin {min(margins):.2e}")

    # removal: frame 0's cloud against three of its boxes as accepted candidates
    rm = np.array([0, 4, 5])
    after = ragm.remove_points_in_boxes(out["points_0"].copy(), BOXES0[rm].copy())
    mine = S.paste(out["points_0"], BOXES0[rm], np.zeros(3, np.int64), np.ones(3, bool), np.zeros((0, 4), np.float32), np.zeros(2, np.int64))
    assert np.array_equal(mine, after), "removal differs from the reference"
    assert 0 < after.shape[0] < N0
    out.update(remove_boxes=rm.astype(np.int32), remove_points=after)
    print(f"removal: {N0 - after.shape[0]} points dropped")
    save("gtsample_small", **out)


if __name__ == "__main__":
    main()
