"""Inputs and CPU references for the post-processing path tests (numpy only; shared by test_postprocess_paths_cpu.py, which
asserts on the oracle alone that every case reaches the path it is named after, and test_postprocess_paths_gpu.py, which
compares the HIP kernels with the oracle on the same inputs).

Geometry: eight_20cm on a 192 x 160 cell grid -> 96 x 80 feature map, A = 69 120 anchors, class ranges [0, 46080),
[46080, 53760), [53760, 69120) (6 / 1 / 2 anchors per location).  The smallest class has 7 680 anchors: more than the 4096
keys of the device's short list, so every class can overflow it.

Every reference is computed once per process and must not be modified by its readers."""
import functools

import numpy as np

from conftest import load_pkg
from oracle import c_oracle as C
from oracle import pp_oracle as O

F32 = np.float32
GX, GY = 192, 160
A = 69120
CLASS_RANGES = ((0, 46080), (46080, 53760), (53760, 69120))

# device constants the path predictions below restate (csrc/postprocess.hip)
NBINS = 4096
SHORT_CAP = 4096
GATHER_BLOCK = 4096   # candidates one post_gather workgroup scans
GATHER_LDS = 1024     # keys it stages in LDS before it appends directly
NMS_AHEAD = 16        # column tiles nms_greedy_wave prefetches; tiles further ahead go through the far-tile fold


def small_config(synth):
    """The small_cfg idiom of tests/test_gpu_parity.py, without the device entry."""
    cfg = synth.load_config("eight_20cm")
    cfg["detection_range"] = [0.0, 0.0, -2.5, 0.2 * GX, 0.2 * GY, 8.5]
    cfg["max_voxels"] = 2000
    return cfg


@functools.lru_cache(maxsize=None)
def geometry():
    cfg = small_config(load_pkg("synth"))
    a = O.make_anchors(O.voxel_setup(cfg))
    assert a["anchors"].shape[0] == A and tuple(tuple(v) for v in a["class_masks"].values()) == CLASS_RANGES
    return dict(anchors=a["anchors"], class_masks=a["class_masks"], center_limit=cfg["center_limit"])


@functools.lru_cache(maxsize=None)
def recipe_r(seed):
    """Tie-free logits on a shuffled grid in [-4, 4), random box / direction logits, 90 % of the anchors masked in."""
    rng = np.random.default_rng(seed)
    logits = rng.permutation(A).astype(F32) / A * 8 - 4
    box = (rng.standard_normal((A, 7)) * 0.3).astype(F32)
    dr = rng.standard_normal((A, 2)).astype(F32)
    mask = rng.random(A) < 0.9
    return logits.astype(F32), box, dr, mask


# ------------------------------------------------------------------ NMS-depth cases
# id -> (pre_max, post_max, iou threshold, mode, seed).  The seeds of the rotated rows were chosen on the CPU: the reference's
# smallest |IoU - threshold| is >= 1e-4 there (test_postprocess_paths_cpu.py asserts it).
NMS_CASES = {
    "far-aabb-s5": (1153, 1024, 0.5, "aabb", 5),
    "far-aabb-s6": (1153, 1024, 0.5, "aabb", 6),
    "far-rot-s5": (1153, 1024, 0.5, "rotated", 5),
    "far-rot-s6": (1153, 1024, 0.5, "rotated", 6),
    "max-aabb-s5": (4096, 1024, 0.5, "aabb", 5),
    "mid-rot-s5": (2500, 700, 0.6, "rotated", 5),
    "mid-rot-s6": (2500, 700, 0.6, "rotated", 6),
    "max-rot-s5": (4096, 1024, 0.7, "rotated", 5),
    "tile-aabb-40": (40, 40, 0.5, "aabb", 5),
    "tile-rot-40": (40, 40, 0.5, "rotated", 5),
    "tile-aabb-64-1": (64, 1, 0.5, "aabb", 5),
    "tile-rot-64-1": (64, 1, 0.5, "rotated", 5),
    "default-aabb": (1000, 300, 0.1, "aabb", 5),
}


@functools.lru_cache(maxsize=None)
def nms_reference(case):
    """(det, counts, info, margin) of the oracle for one NMS case; margin = smallest |IoU - threshold| its NMS saw."""
    pre, post, iou, mode, seed = NMS_CASES[case]
    logits, box, dr, mask = recipe_r(seed)
    g = geometry()
    with C.numba_typing(False) as nt:
        det, counts, info = O.postprocess(logits, box, dr, mask, g["anchors"], g["class_masks"], g["center_limit"], mode, detail=True,
                                          nms_fn=C.nms_rotated if mode == "rotated" else C.nms_aabb, pre_max=pre, post_max=post, iou_thr=iou)
    return det, counts, info, nt.margin


def last_emitted(info_c, post_max):
    """Position in score order of the last row the sweep emits (-1: none), and whether the post_max cut was reached."""
    keep = info_c["keep"]
    if keep.size == 0:
        return -1, False
    return int(keep[:post_max][-1]), keep.size >= post_max


# ------------------------------------------------------------------ selection cases
SELECT_PARAMS = ((1000, 0.05), (4096, 0.05), (1153, 0.5), (1000, 1e-4), (64, 0.999))
SELECT_CASES = ("S1-ties", "S2-all-equal", "S3-counts-a", "S3-counts-b", "S4-boundary", "S5-one-bin", "S6-saturated")
SELECT_SEED = 5


def _ordered(u):
    """uint32 bit pattern of a float32 -> integer that orders like the float."""
    u = int(u)
    return (0x80000000 - (u & 0x7FFFFFFF)) if u & 0x80000000 else (0x80000000 + u)


def _from_ordered(k):
    u = (0x80000000 - k) | 0x80000000 if k < 0x80000000 else k - 0x80000000
    return np.array([u & 0xFFFFFFFF], dtype=np.uint32).view(F32)[0]


def midpoint_margin(x):
    """Relative distance of the fp64 sigmoid of the float32 logit x from the nearest fp32 rounding midpoint."""
    s = 1.0 / (1.0 + np.exp(-np.float64(x)))
    f = F32(s)
    nb = np.nextafter(f, F32(2.0) if np.float64(f) < s else F32(-1.0))
    mid = (np.float64(f) + np.float64(nb)) / 2.0
    return abs(s - mid) / s


@functools.lru_cache(maxsize=None)
def boundary_pair(thr):
    """(hi, lo, margin): hi = the smallest float32 logit whose fp32 score is >= thr, lo = the float32 just below it (its score
    is < thr), margin = the smaller midpoint_margin of the two -- an fp64 exp that differs in its last bit moves the sigmoid by
    ~1e-16 relative, so with margin >= 1e-9 neither score can round differently on the device."""
    t = F32(thr)
    lo_k, hi_k = _ordered(F32(-30.0).view(np.uint32)), _ordered(F32(30.0).view(np.uint32))
    assert O.sigmoid_f32(_from_ordered(lo_k)) < t <= O.sigmoid_f32(_from_ordered(hi_k))
    while hi_k - lo_k > 1:  # sigmoid_f32 is monotone: bisect on the ordered bit patterns
        m = (lo_k + hi_k) // 2
        if O.sigmoid_f32(_from_ordered(m)) >= t:
            hi_k = m
        else:
            lo_k = m
    hi, lo = _from_ordered(hi_k), _from_ordered(lo_k)
    return hi, lo, min(midpoint_margin(hi), midpoint_margin(lo))


def s4_usable(thr):
    return boundary_pair(thr)[2] >= 1e-9


def _logit(p):
    return float(np.log(p) - np.log1p(-p))


@functools.lru_cache(maxsize=None)
def select_inputs(case, pre_max, thr):
    """(logits, mask) of one selection case, or None where the case does not exist at this threshold (S4 without a safe pair)."""
    base, _, _, mask = recipe_r(SELECT_SEED)
    rng = np.random.default_rng(1000 + SELECT_CASES.index(case))
    K = pre_max
    if case == "S1-ties":
        logits = (np.round(base * 8) / 8).astype(F32)
    elif case == "S2-all-equal":
        logits = np.zeros(A, F32)
    elif case.startswith("S3"):
        # exactly n passing, masked-in anchors per class; distinct logits from 0.5 above the threshold's logit
        ns = (0, K - 1, K + 1) if case.endswith("a") else (K, 1, K)
        logits = np.full(A, -20.0, F32)
        for (s, e), n in zip(CLASS_RANGES, ns):
            ids = rng.choice(np.nonzero(mask[s:e])[0] + s, n, replace=False)
            logits[ids] = rng.permutation(np.linspace(_logit(thr) + 0.5, _logit(thr) + 4.5, max(n, 1))[:n]).astype(F32)
    elif case == "S4-boundary":
        if not s4_usable(thr):
            return None
        hi, lo, _ = boundary_pair(thr)
        logits = np.full(A, -20.0, F32)
        for s, e in CLASS_RANGES:
            ids = rng.choice(np.nonzero(mask[s:e])[0] + s, 600, replace=False)
            logits[ids[:300]] = hi
            logits[ids[300:]] = lo
    elif case == "S5-one-bin":
        logits = np.empty(A, F32)
        for s, e in CLASS_RANGES:
            logits[s:e] = rng.permutation(np.linspace(-0.0015, 0.0015, e - s)).astype(F32)
    elif case == "S6-saturated":
        logits = base.copy()
        for s, e in CLASS_RANGES:
            logits[rng.choice(np.arange(s, e), 5000, replace=False)] = 20.0
    else:
        raise KeyError(case)
    logits.setflags(write=False)
    return logits, mask


@functools.lru_cache(maxsize=None)
def select_reference(case, pre_max, thr):
    """Per class dict(idx, score, n_cand) of the oracle's selection (postprocess(detail=True)), or None (see select_inputs)."""
    inp = select_inputs(case, pre_max, thr)
    if inp is None:
        return None
    logits, mask = inp
    _, box, dr, _ = recipe_r(SELECT_SEED)
    g = geometry()
    _, _, info = O.postprocess(logits, box, dr, mask, g["anchors"], g["class_masks"], g["center_limit"], "aabb", detail=True,
                               nms_fn=C.nms_aabb, pre_max=pre_max, post_max=1, iou_thr=0.5, score_thr=thr)
    return [dict(idx=np.asarray(i["idx"], np.int64), score=np.asarray(i["score"], F32), n_cand=int(i["n_cand"])) for i in info]


# ------------------------------------------------------------------ which device path a class takes (restated from the kernels)
def shift_for(thr):
    rng_ = 0x3F800000 - int(F32(thr).view(np.uint32))
    s = 0
    while (rng_ >> s) >= NBINS:
        s += 1
    return s


def predicted_path(logits, mask, c, pre_max, thr):
    """The selection path class c takes on the device, from its candidates' coarse score bins: dict(total, path, short, direct) with
    path = 'none' (no candidate) | 'all' (total <= K: everything is taken) | 'short' (the short list holds the bins from the K-th
    score's upwards) | 'radix' (those bins hold more than SHORT_CAP keys: radix select over the whole candidate list);
    short = number of keys in those bins; direct = those bins hold more than 1024 keys per 4096-candidate block on AVERAGE, so
    whatever the candidates' order at least one post_gather workgroup overflows its LDS buffer and appends directly."""
    s, e = CLASS_RANGES[c]
    sc = O.sigmoid_f32(logits[s:e][mask[s:e]])
    sc = sc[sc >= F32(thr)]
    total = int(sc.size)
    if total == 0:
        return dict(total=0, path="none", short=0, direct=False)
    bins = np.minimum((sc.view(np.uint32).astype(np.int64) - int(F32(thr).view(np.uint32))) >> shift_for(thr), NBINS - 1)
    if total <= pre_max:
        short = total
        path = "all"
    else:
        hist = np.bincount(bins, minlength=NBINS)[::-1].cumsum()[::-1]  # hist[b] = candidates in bins >= b
        tb = int(np.nonzero(hist >= pre_max)[0].max())
        short = int(hist[tb])
        path = "radix" if short > SHORT_CAP else "short"
    nblocks = -(-total // GATHER_BLOCK)
    return dict(total=total, path=path, short=short, direct=short > GATHER_LDS * nblocks)
