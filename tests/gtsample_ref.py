"""Numpy restatement of ground-truth database sampling (csrc/gt_sample.hip, framework/gt_sampler.py): count / extract / select /
paste on top of tests/augment_ref.py's face planes and box_collision_test, in the kernels' float32 order, and the sampler's host
logic.  Held to the reference's points_in_rbbox / box_collision_test / remove_points_in_boxes by tests/golden/gtsample_small.npz.
Every comparison records its distance from the threshold in `margins` when one is passed."""
import numpy as np

import augment_ref as R

F32 = np.float32
MAX_BOXES = 256  # PP_AUG_MAX_BOXES
DIFFICULTY_EXTRA = (1.2, 0.5, 8.0)


def grown(boxes, extra=(0.0, 0.0, 0.0)):
    """(l, w, h) + extra in float32, as pp_gt_count adds it."""
    b = np.asarray(boxes, F32).reshape(-1, 7).copy()
    b[:, 3:6] = b[:, 3:6] + np.asarray(extra, F32)
    return b


def signs(points, box):
    """f32[M,6]: the six face-plane signs of every point for one box."""
    pl = R.face_planes(np.asarray(box, F32))
    p = np.asarray(points, F32)
    return ((p[:, 0:1] * pl[:, 0] + p[:, 1:2] * pl[:, 1]) + p[:, 2:3] * pl[:, 2]) + pl[:, 3]


def member_table(points, boxes, extra=(0.0, 0.0, 0.0), margins=None):
    """bool[M,N]: points_in_rbbox (origin 0.5, 0.5, 0.5), inside at sign < 0 on all six faces."""
    b = grown(boxes, extra)
    out = np.zeros((np.asarray(points).shape[0], b.shape[0]), bool)
    for j in range(b.shape[0]):
        sg = signs(points, b[j])
        if margins is not None and sg.size:
            margins.append(float(np.abs(sg).min()))
        out[:, j] = (sg < 0).all(axis=1)
    return out


def count(points, boxes, extra=(0.0, 0.0, 0.0)):
    return member_table(points, boxes, extra).sum(axis=0).astype(np.int32)


def extract(points, boxes):
    """-> (local f32[T,4], off i64[N+1]): per box its member points in the cloud's order, xyz minus the centre in float32."""
    p = np.asarray(points, F32).reshape(-1, 4)
    b = np.asarray(boxes, F32).reshape(-1, 7)
    tab = member_table(p, b)
    parts = []
    for j in range(b.shape[0]):
        q = p[tab[:, j]].copy()
        q[:, :3] = q[:, :3] - b[j, :3]
        parts.append(q)
    off = np.concatenate([[0], np.cumsum([q.shape[0] for q in parts])]).astype(np.int64)
    return (np.concatenate(parts) if parts else np.zeros((0, 4), F32)).astype(F32), off


def corners(box):
    return R.bev_corners(*np.asarray(box, F32)[[0, 1, 3, 4, 6]])


def collision_matrix(cand, others, containment=True, margins=None, contained=None):
    """bool[Nc,No]: box_collision_test(candidate corners, other corners)."""
    cand, others = np.asarray(cand, F32).reshape(-1, 7), np.asarray(others, F32).reshape(-1, 7)
    out = np.zeros((cand.shape[0], others.shape[0]), bool)
    for i in range(cand.shape[0]):
        for k in range(others.shape[0]):
            out[i, k] = R.collide(corners(cand[i]), corners(others[k]), containment, margins, contained)
    return out


def select(existing, cand, containment=True, margins=None, contained=None):
    """bool[Nc]: candidate j accepted iff it collides with no existing box and no earlier ACCEPTED candidate."""
    existing, cand = np.asarray(existing, F32).reshape(-1, 7), np.asarray(cand, F32).reshape(-1, 7)
    acc = np.zeros(cand.shape[0], bool)
    for j in range(cand.shape[0]):
        cj = corners(cand[j])
        hit = any(R.collide(cj, corners(e), containment, margins, contained) for e in existing)
        hit = hit or any(acc[k] and R.collide(cj, corners(cand[k]), containment, margins, contained) for k in range(j))
        acc[j] = not hit
    return acc


def paste(points, cand, cand_idx, accept, db_points, db_off, remove=True, margins=None):
    """One frame: the accepted objects in candidate order (local + centre, float32), then the surviving scene points."""
    p = np.asarray(points, F32).reshape(-1, 4)
    cand = np.asarray(cand, F32).reshape(-1, 7)
    n_db = len(db_off) - 1
    ok = [bool(accept[j]) and 0 <= int(cand_idx[j]) < n_db for j in range(cand.shape[0])]
    parts = []
    for j in range(cand.shape[0]):
        if ok[j]:
            q = np.asarray(db_points, F32)[db_off[cand_idx[j]]:db_off[cand_idx[j] + 1]].copy()
            q[:, :3] = q[:, :3] + cand[j, :3]
            parts.append(q)
    keep = np.ones(p.shape[0], bool)
    if remove and any(ok):
        keep = ~member_table(p, cand[np.array(ok)], margins=margins).any(axis=1)
    return np.concatenate(parts + [p[keep]]).astype(F32)


# ---------------------------------------------------------------------------------------------- the sampler's host logic
def k_counts(targets, gt_classes, n_per_class):
    """k_c = min(max(target_c - existing boxes of class c, 0), n_c); gt_classes 1-based."""
    C = len(targets)
    have = np.array([(np.asarray(gt_classes) == c + 1).sum() for c in range(C)], np.int64)
    return np.minimum(np.maximum(np.asarray(targets, np.int64) - have, 0), np.asarray(n_per_class, np.int64))


def cut(k, n_existing, cap=MAX_BOXES):
    """The candidate list (class order, then draw order) cut so that existing + candidates <= cap: the counts kept."""
    room = max(cap - n_existing, 0)
    out = []
    for v in k:
        out.append(min(int(v), room))
        room -= out[-1]
    return np.array(out, np.int64)


def draw_numpy(targets, gt_classes, class_off):
    """The numpy-mode draws by hand: np.random.choice(n_c, k_c, replace=False) per class with k_c > 0, then the cut."""
    n = np.diff(class_off)
    k = k_counts(targets, gt_classes, n)
    kept = cut(k, len(gt_classes))
    rows = []
    for c in range(len(k)):
        if k[c] > 0:
            rows.append(class_off[c] + np.random.choice(int(n[c]), int(k[c]), replace=False)[:kept[c]])
    return np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
