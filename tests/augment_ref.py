"""Numpy restatement of the training-input augmentation (reference augmentation.py, box_np_ops.py:6-16,102-104,460-467 and
dataset.py:121-146) in the reference's float32 / float64 order, for csrc/augment.hip.  Box collisions follow numba's semantics of
`ret[i, j] is True / is False` (value tests): containment without an edge crossing is a collision.  `containment=False` gives the
plain-Python semantics (the branch never runs).  Every comparison records its margin in `margins` when one is passed."""
import numpy as np

F32 = np.float32
NX = np.array([-0.5, -0.5, 0.5, 0.5], F32)
NY = np.array([-0.5, 0.5, 0.5, -0.5], F32)


def bev_corners(x, y, l, w, r):
    """box2d_to_corner_jit of one box: f32[4,2]."""
    s, c = np.sin(F32(r)), np.cos(F32(r))
    cx, cy = F32(l) * NX, F32(w) * NY
    return np.stack([(cx * c + cy * (-s)) + F32(x), (cx * s + cy * c) + F32(y)], axis=1)


def standup(c):
    return np.array([c[:, 0].min(), c[:, 1].min(), c[:, 0].max(), c[:, 1].max()], F32)


def _gt(a, b, margins):
    if margins is not None:
        margins.append(abs(float(a) - float(b)))
    return a > b


def _inside_all(b, q, margins):
    for l in range(4):
        for k in range(4):
            k1 = (k + 1) % 4
            v = -(b[k] - b[k1])
            cross = v[1] * (b[k, 0] - q[l, 0])
            cross = cross - v[0] * (b[k, 1] - q[l, 1])
            if margins is not None:
                margins.append(abs(float(cross)))
            if cross >= 0:
                return False
    return True


def collide(b, q, containment=True, margins=None, contained=None):
    bs, qs = standup(b), standup(q)
    iw = min(bs[2], qs[2]) - max(bs[0], qs[0])
    if margins is not None:
        margins.append(abs(float(iw)))
    if not iw > 0:
        return False
    ih = min(bs[3], qs[3]) - max(bs[1], qs[1])
    if margins is not None:
        margins.append(abs(float(ih)))
    if not ih > 0:
        return False
    for k in range(4):
        A, B = b[k], b[(k + 1) % 4]
        for l in range(4):
            C, D = q[l], q[(l + 1) % 4]
            acd = _gt((D[1] - A[1]) * (C[0] - A[0]), (C[1] - A[1]) * (D[0] - A[0]), margins)
            bcd = _gt((D[1] - B[1]) * (C[0] - B[0]), (C[1] - B[1]) * (D[0] - B[0]), margins)
            if acd != bcd:
                abc = _gt((C[1] - A[1]) * (B[0] - A[0]), (B[1] - A[1]) * (C[0] - A[0]), margins)
                abd = _gt((D[1] - A[1]) * (B[0] - A[0]), (B[1] - A[1]) * (D[0] - A[0]), margins)
                if abc != abd:
                    return True
    inside = _inside_all(b, q, margins) or _inside_all(q, b, margins)
    if inside and contained is not None:
        contained.append(True)
    return inside and containment


def noise_select(boxes, valid, loc, rot, grot, containment=True, margins=None, contained=None):
    """noise_per_box_v2_ + _select_transform: boxes f32[N,7] -> sel i64[N], sel_loc f64[N,3], sel_rot f64[N]."""
    n = boxes.shape[0]
    T = loc.shape[1] if loc.ndim == 3 else 0
    corners = [bev_corners(*boxes[i, [0, 1, 3, 4, 6]]) for i in range(n)]
    sel = -np.ones(n, np.int64)
    sel_loc = np.zeros((n, 3))
    sel_rot = np.zeros(n)
    for i in range(n):
        if not valid[i]:
            continue
        x, y, l, w, r = boxes[i, [0, 1, 3, 4, 6]]
        rad = np.sqrt(x * x + y * y)
        cg = np.arctan2(y, x)
        for j in range(T):
            dg = np.float64(cg) + grot[i, j]
            dpx, dpy = F32(np.float64(rad) * np.cos(dg)), F32(np.float64(rad) * np.sin(dg))
            cr = F32(np.float64(r) + grot[i, j])
            rs, rc = np.sin(cr), np.cos(cr)
            ns, nc = F32(np.sin(rot[i, j])), F32(np.cos(rot[i, j]))
            cx, cy = l * NX, w * NY
            x1, y1 = cx * rc + cy * (-rs), cx * rs + cy * rc
            x2, y2 = x1 * nc + y1 * (-ns), x1 * ns + y1 * nc
            ox, oy = np.float64(dpx) + loc[i, j, 0], np.float64(dpy) + loc[i, j, 1]
            c = np.stack([(x2.astype(np.float64) + ox).astype(F32), (y2.astype(np.float64) + oy).astype(F32)], axis=1)
            if not any(collide(c, corners[k], containment, margins, contained) for k in range(n) if k != i):
                sel[i] = j
                corners[i] = c
                sel_loc[i] = loc[i, j]
                sel_loc[i, 0] += np.float64(dpx - x)
                sel_loc[i, 1] += np.float64(dpy - y)
                sel_rot[i] = rot[i, j] + (dg - np.float64(cg))
                break
    return sel, sel_loc, sel_rot


def _rot(a):
    return F32(np.cos(a)), F32(np.sin(a))


def global_rotate(v, flip, pitch, roll, yaw, rotate=True):
    """v f32[M,3] -> f32[M,3]: random_flip then the three rotation_points_single_angle calls."""
    x, y, z = v[:, 0].copy(), v[:, 1].copy(), v[:, 2].copy()
    if flip:
        y = -y
    if rotate:
        c, s = _rot(pitch)
        x, z = x * c + z * (-s), x * s + z * c
        c, s = _rot(roll)
        y, z = y * c + z * s, y * (-s) + z * c
        c, s = _rot(yaw)
        x, y = x * c + y * (-s), x * s + y * c
    return np.stack([x, y, z], axis=1)


def boxes_chain(boxes, valid, sel_loc, sel_rot, prm, bv_range):
    """The box side (box3d_transform_, flip, rotation, scaling, translation, range filter, limit_period) of one frame:
    -> (boxes f32[N,7] after the chain, keep bool[N])."""
    st = int(prm[0])
    b = boxes.astype(F32).copy()
    if st & 1:
        m = np.asarray(valid, bool)
        b[m, :3] = (b[m, :3].astype(np.float64) + sel_loc[m]).astype(F32)
        b[m, 6] = (b[m, 6].astype(np.float64) + sel_rot[m]).astype(F32)
    flip = (st & 2) and prm[1] != 0
    if flip:
        b[:, 6] = -b[:, 6]
    b[:, :3] = global_rotate(b[:, :3], flip, prm[2], prm[3], prm[4], bool(st & 4))
    if st & 4:
        b[:, 6] = b[:, 6] + F32(prm[4])
    if st & 8:
        b[:, :3] = (b[:, :3].astype(np.float64) * prm[5:8]).astype(F32)
        fx, fy = F32(prm[5]), F32(prm[6])
        cr, sr = np.cos(b[:, 6]), np.sin(b[:, 6])
        b[:, 3] = b[:, 3] * np.sqrt(np.square(fx * cr) + np.square(fy * sr))
        b[:, 4] = b[:, 4] * np.sqrt(np.square(fx * sr) + np.square(fy * cr))
        b[:, 5] = b[:, 5] * F32(prm[7])
        b[:, 6] = np.arctan(np.tan(b[:, 6]) * F32(prm[6] / prm[5]))
    if st & 16:
        b[:, :3] = (b[:, :3].astype(np.float64) + prm[8:11]).astype(F32)
    keep = np.ones(b.shape[0], bool)
    if st & 32:
        keep = in_range(b, bv_range)
        tp = F32(2 * np.pi)
        b[:, 6] = b[:, 6] - np.floor(b[:, 6] / tp + F32(0.5)) * tp
    return b, keep


def in_range(b, rg):
    """kitti_io.gt_in_range: some BEV corner strictly inside the clockwise range rectangle."""
    x0, y0, x1, y1 = [F32(v) for v in rg]
    poly = np.array([[x0, y0], [x0, y1], [x1, y1], [x1, y0]], F32)
    vec = poly - poly[[3, 0, 1, 2]]
    out = np.zeros(b.shape[0], bool)
    for i in range(b.shape[0]):
        c = bev_corners(*b[i, [0, 1, 3, 4, 6]])
        ins = np.ones(4, bool)
        for k in range(4):
            ins &= vec[k, 1] * (poly[k, 0] - c[:, 0]) - vec[k, 0] * (poly[k, 1] - c[:, 1]) < 0
        out[i] = ins.any()
    return out


def face_planes(b):
    """points_in_rbbox's planes of one box (origin 0.5, 0.5, 0.5): f32[6,4] (normal, -d)."""
    s, c = np.sin(F32(b[6])), np.cos(F32(b[6]))
    u = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 0, 0], [1, 0, 1], [1, 1, 1], [1, 1, 0]], F32) - F32(0.5)
    d = b[3:6].astype(F32) * u
    cx = (d[:, 0] * c + d[:, 1] * (-s)) + b[0]
    cy = (d[:, 0] * s + d[:, 1] * c) + b[1]
    cz = d[:, 2] + b[2]
    P = np.stack([cx, cy, cz], axis=1).astype(F32)
    out = np.zeros((6, 4), F32)
    for q, (i0, i1, i2) in enumerate([(0, 1, 2), (7, 6, 5), (0, 3, 7), (1, 5, 6), (0, 4, 5), (3, 2, 6)]):
        a, bb = P[i0] - P[i1], P[i1] - P[i2]
        n = np.array([a[1] * bb[2] - a[2] * bb[1], a[2] * bb[0] - a[0] * bb[2], a[0] * bb[1] - a[1] * bb[0]], F32)
        out[q, :3] = n
        out[q, 3] = -((n[0] * P[i0, 0] + n[1] * P[i0, 1]) + n[2] * P[i0, 2])
    return out


def membership(points, boxes, valid, margins=None):
    """Index of the first VALID box containing each point (original boxes), -1 if none: i64[M]."""
    m = points.shape[0]
    owner = -np.ones(m, np.int64)
    for j in range(boxes.shape[0]):
        pl = face_planes(boxes[j])
        sg = ((points[:, 0:1] * pl[:, 0] + points[:, 1:2] * pl[:, 1]) + points[:, 2:3] * pl[:, 2]) + pl[:, 3]
        if margins is not None and sg.size:
            margins.append(float(np.abs(sg).min()))
        if not valid[j]:
            continue
        inside = (sg < 0).all(axis=1) & (owner < 0)
        owner[inside] = j
    return owner


def points_chain(points, boxes, valid, sel_loc, sel_rot, prm, perm=None, margins=None):
    """The point side of one frame: f32[M,4] -> f32[M,4] (row k = source row perm[k])."""
    st = int(prm[0])
    p = points.astype(F32).copy()
    if st:
        v = p[:, :3].copy()
        if st & 1 and boxes.shape[0]:
            owner = membership(v, boxes, valid, margins)
            for j in np.unique(owner[owner >= 0]):
                sel = owner == j
                c, s = _rot(sel_rot[j])
                ctr = boxes[j, :3].astype(F32)
                d = v[sel] - ctr
                rx, ry = d[:, 0] * c + d[:, 1] * (-s), d[:, 0] * s + d[:, 1] * c
                w = np.stack([rx, ry, d[:, 2]], axis=1) + ctr
                v[sel] = (w.astype(np.float64) + sel_loc[j]).astype(F32)
        v = global_rotate(v, (st & 2) and prm[1] != 0, prm[2], prm[3], prm[4], bool(st & 4))
        if st & 8:
            v = (v.astype(np.float64) * prm[5:8]).astype(F32)
        if st & 16:
            v = (v.astype(np.float64) + prm[8:11]).astype(F32)
        p[:, :3] = v
    return p if perm is None else p[perm]
