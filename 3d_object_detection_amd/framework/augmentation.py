"""framework.augmentation (reference augmentation.py): the training-input augmentation of GenericDataset.__getitem__.

The random draws stay on the host and consume the global legacy np.random stream exactly as the reference does (`draw_frame`);
everything whose cost grows with points or tries runs in csrc/augment.hip.  The reference-named functions work in place on numpy
arrays (as the reference's do) or on device tensors, draw what the reference draws, and run through the same kernels."""
import numpy as np
import torch

from .. import _lib

# noise_per_object's defaults as dataset.py:127 calls it (augmentation.py:177-183)
ROTATION_PERTURB = (5.0 / 180) * np.pi
CENTER_NOISE_STD = 0.15
GLOBAL_RANDOM_ROT_RANGE = (2.0 / 180) * np.pi
NUM_TRY = 100
NOISE_TRANSLATE_STD = (0.25, 0.25, 0.25)  # dataset.py:133

# prm layout (include/pp_hip.h PP_AUG_*) and the step bits of prm[P_ON] (csrc/augment.hip ST_*)
P_ON, P_FLIP, P_PITCH, P_ROLL, P_YAW, P_SX, P_SY, P_SZ, P_TX, P_TY, P_TZ = range(11)
ST_MOVE, ST_FLIP, ST_ROT, ST_SCALE, ST_TRANS, ST_RANGE, ST_PERM = 1, 2, 4, 8, 16, 32, 64
P_KEY_LO, P_KEY_HI = 11, 12
ST_AUGM = ST_MOVE | ST_FLIP | ST_ROT | ST_SCALE | ST_TRANS


def identity_params(steps=0):
    """f64[PP_AUG_PARAMS]: the given steps with neutral values (no flip, zero angles, unit scales, zero translation)."""
    p = np.zeros(_lib.PP_AUG_PARAMS, np.float64)
    p[P_ON] = steps
    p[P_SX:P_SZ + 1] = 1.0
    return p


# ---------------------------------------------------------------------------------------------- draws (host, the reference's order)
def draw_noise(n_boxes, num_try=NUM_TRY):
    """noise_per_object's three draws (augmentation.py:191-194): loc f64[N,T,3], rot f64[N,T], grot f64[N,T].  N = 0 draws nothing."""
    std = np.array([CENTER_NOISE_STD] * 3, dtype=np.float32)  # center_noise_std in gt_boxes.dtype
    loc = np.random.normal(scale=std, size=[n_boxes, num_try, 3])
    rot = np.random.uniform(-ROTATION_PERTURB, ROTATION_PERTURB, size=[n_boxes, num_try])
    grot = np.random.uniform(-GLOBAL_RANDOM_ROT_RANGE, GLOBAL_RANDOM_ROT_RANGE, size=[n_boxes, num_try])
    return loc, rot, grot


def draw_flip():
    return 1.0 if np.random.random() > 0.5 else 0.0  # random_flip (:10)


def draw_rotation():
    """global_rotation_v2 (:29-48): pitch U(+-4 deg), roll U(+-2 deg), yaw U(+-30 deg), as `deg / 180 * np.pi`."""
    pitch = np.random.uniform(-4, 4) / 180 * np.pi
    roll = np.random.uniform(-2, 2) / 180 * np.pi
    yaw = np.random.uniform(-30, 30) / 180 * np.pi
    return pitch, roll, yaw


def draw_scaling():
    """global_scaling_v2 (:57-61): its min / max arguments are ignored by the reference."""
    return np.random.uniform(0.9, 1.1), np.random.uniform(0.9, 1.1), np.random.uniform(0.95, 1.05)


def draw_translate(noise_translate_std=NOISE_TRANSLATE_STD):
    """global_translate (:82-84): three separate normal(0, std, 1) draws."""
    if not isinstance(noise_translate_std, (list, tuple, np.ndarray)):
        noise_translate_std = [noise_translate_std] * 3
    return tuple(float(np.random.normal(0, noise_translate_std[k], 1)[0]) for k in range(3))


def draw_frame(n_points, n_boxes, training=True, augm=True, num_try=NUM_TRY):
    """Every draw GenericDataset.__getitem__ makes for one frame, in its order (dataset.py:121-146): noise_per_object, random_flip,
    global_rotation_v2, global_scaling_v2, global_translate (training and augm only), then the shuffle (training only), drawn as
    np.random.permutation(n) -- the same draws as np.random.shuffle, and points[perm] equals the shuffled array.
    Returns dict(loc, rot, grot, prm f64[PP_AUG_PARAMS], perm int64[n] or None)."""
    prm = identity_params(0)
    loc = np.zeros((n_boxes, num_try, 3))
    rot = np.zeros((n_boxes, num_try))
    grot = np.zeros((n_boxes, num_try))
    perm = None
    if training:
        if augm:
            loc, rot, grot = draw_noise(n_boxes, num_try)
            prm[P_FLIP] = draw_flip()
            prm[P_PITCH:P_YAW + 1] = draw_rotation()
            prm[P_SX:P_SZ + 1] = draw_scaling()
            prm[P_TX:P_TZ + 1] = draw_translate()
            prm[P_ON] = ST_AUGM | ST_RANGE
        else:
            prm[P_ON] = ST_RANGE
        perm = np.random.permutation(n_points)
    return dict(loc=loc, rot=rot, grot=grot, prm=prm, perm=perm)


# ---------------------------------------------------------------------------------------------- device runs
_OWN = {}


def _engine(device=None):
    """The augmentation kernels need a context only for error reporting: use a live engine, else one built from the shipped
    eight_20cm config (kept alive here)."""
    from ..engine import _ENGINES, engine_for
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    live = [e for e in list(_ENGINES) if getattr(e, "ctx", None) and e.device.index == (dev.index or 0)]
    if live:
        return live[-1]
    if dev not in _OWN:
        from .. import synth
        cfg = synth.load_config("eight_20cm")
        cfg["device"] = dev
        _OWN[dev] = cfg
    return engine_for(_OWN[dev])


def frame_steps(training=True, augm=True, device=False):
    """prm[P_ON] of a dataset frame: the whole chain (augm) or the range filter only, plus the inline permutation in device mode."""
    if not training:
        return 0
    return (ST_AUGM | ST_RANGE if augm else ST_RANGE) | (ST_PERM if device else 0)


def draw_device(eng, seed, epoch, samples, box_off, training=True, augm=True, num_try=NUM_TRY):
    """Device random mode: the draws of draw_frame for nb frames from Philox4x32-10 keyed by (seed, epoch, sample index), written
    on the device (no host draws, no permutation upload; the shuffle is a keyed Feistel bijection evaluated by the points kernel).
    Returns a dict of device tensors loc f64[G,T,3], rot / grot f64[G,T], prm f64[nb,PP_AUG_PARAMS], for run_frames."""
    steps = frame_steps(training, augm, True)
    loc, rot, grot, prm = eng.augment_draw(seed, epoch, samples, steps, box_off, num_try)
    return dict(loc=loc, rot=rot, grot=grot, prm=prm, steps=steps, box_counts=[int(b) - int(a) for a, b in zip(box_off, box_off[1:])])


def export_device_draws(eng, d, pt_off):
    """Test hook: the records of draw_device as host draw_frame dicts, the permutation included (evaluated by the points kernel on
    an iota cloud, so it is the kernel's own).  Fed through the numpy-mode path they give the device mode's output bit for bit."""
    nb = int(d["prm"].shape[0])
    n = [pt_off[f + 1] - pt_off[f] for f in range(nb)]
    if max(n + [0]) >= 1 << 24:
        raise ValueError("export_device_draws: frames of 2^24 points or more")
    prm = d["prm"].cpu().numpy()
    iota = torch.zeros((int(pt_off[-1]), 4), dtype=torch.float32, device=eng.device)
    for f in range(nb):
        iota[pt_off[f]:pt_off[f + 1], 0] = torch.arange(n[f], dtype=torch.float32, device=eng.device)
    pp = np.stack([identity_params(ST_PERM) for _ in range(nb)])
    pp[:, P_KEY_LO:P_KEY_HI + 1] = prm[:, P_KEY_LO:P_KEY_HI + 1]
    e = torch.zeros(0, device=eng.device)
    src = eng.augment_points(iota, None, pt_off, e.reshape(0, 7).float(), e.to(torch.uint8), e.reshape(0, 3).double(), e.double(),
                             torch.from_numpy(pp).to(eng.device), [0] * (nb + 1))[:, 0].cpu().numpy().astype(np.int64)
    G = int(d["loc"].shape[0])
    loc, rot, grot = d["loc"].cpu().numpy(), d["rot"].cpu().numpy(), d["grot"].cpu().numpy()
    out, g0 = [], 0
    boxes_per = d.get("box_counts")
    for f in range(nb):
        rec = dict(prm=prm[f].copy(), perm=src[pt_off[f]:pt_off[f + 1]] if int(prm[f, P_ON]) & ST_PERM else None)
        rec["prm"][P_ON] = int(prm[f, P_ON]) & ~ST_PERM
        gn = boxes_per[f] if boxes_per is not None else G
        rec.update(loc=loc[g0:g0 + gn], rot=rot[g0:g0 + gn], grot=grot[g0:g0 + gn])
        g0 += gn
        out.append(rec)
    return out


def run_frames(eng, points, pt_off, boxes, classes, valid, box_off, draws, bv_range):
    """One set of augmentation launches over nb frames.  points f32[P,4] / boxes f32[G,7] / classes i32[G] / valid u8[G] device
    tensors with host CSR offsets; draws: nb host records of draw_frame (numpy mode) or one dict of draw_device (device mode).
    Returns (points f32[P,4], boxes f32[G,7] kept-first per frame, classes i32[G], keep u8[G], kept i32[nb], sel i32[G]), all on
    the device, no host sync."""
    dev = eng.device
    G = int(boxes.shape[0])
    perm = None
    if isinstance(draws, dict):  # device mode: parameters already on the device, the permutation evaluated inline
        loc, rot, grot, prm = draws["loc"], draws["rot"], draws["grot"], draws["prm"]
        move = bool(draws["steps"] & ST_MOVE)
    else:
        T = max([int(d["loc"].shape[1]) for d in draws] + [1])
        prm = torch.from_numpy(np.stack([d["prm"] for d in draws])).to(dev)
        move = any(int(d["prm"][P_ON]) & ST_MOVE for d in draws)
        if G and move:
            loc = torch.from_numpy(np.ascontiguousarray(np.concatenate([d["loc"].reshape(-1, T, 3) for d in draws]))).to(dev)
            rot = torch.from_numpy(np.ascontiguousarray(np.concatenate([d["rot"].reshape(-1, T) for d in draws]))).to(dev)
            grot = torch.from_numpy(np.ascontiguousarray(np.concatenate([d["grot"].reshape(-1, T) for d in draws]))).to(dev)
        if any(d["perm"] is not None for d in draws):
            perm = np.concatenate([np.arange(pt_off[f + 1] - pt_off[f]) if d["perm"] is None else d["perm"] for f, d in enumerate(draws)])
            perm = torch.from_numpy(perm.astype(np.int32)).to(dev)
    if G and move:
        sel, sel_loc, sel_rot = eng.augment_noise(boxes, valid, loc, rot, grot, box_off)
    else:
        sel = torch.full((G,), -1, dtype=torch.int32, device=dev)  # no box moves in these frames
        sel_loc = torch.zeros((G, 3), dtype=torch.float64, device=dev)
        sel_rot = torch.zeros(G, dtype=torch.float64, device=dev)
    out_pts = eng.augment_points(points, perm, pt_off, boxes, valid, sel_loc, sel_rot, prm, box_off)
    out_box, out_cls, keep, kept = eng.augment_boxes(boxes, classes, valid, sel_loc, sel_rot, prm, box_off, bv_range)
    return out_pts, out_box, out_cls, keep, kept, sel


def _as_dev(eng, x, dtype):
    if isinstance(x, torch.Tensor):
        return x.to(eng.device, dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(x, dtype=torch.empty(0, dtype=dtype).numpy().dtype)).to(eng.device)


def _apply_one(gt_boxes, points, draws, valid_mask=None):
    """Run one frame's draws through the kernels and write the results back into gt_boxes / points (numpy or device tensors)."""
    ref = gt_boxes if isinstance(gt_boxes, torch.Tensor) else points if isinstance(points, torch.Tensor) else None
    eng = _engine(ref.device if ref is not None and ref.is_cuda else None)
    n_box = int(gt_boxes.shape[0])
    b = _as_dev(eng, gt_boxes, torch.float32).reshape(-1, 7)
    vm = np.ones(n_box, bool) if valid_mask is None else np.asarray(valid_mask, bool)[:n_box]
    v = _as_dev(eng, vm, torch.uint8)
    cls = torch.zeros(n_box, dtype=torch.int32, device=eng.device)
    if points is None:
        p = torch.zeros((0, 4), dtype=torch.float32, device=eng.device)
    else:
        p = _as_dev(eng, points, torch.float32)
        if p.shape[1] != 4:
            raise ValueError("augmentation: points must have 4 features (x, y, z, intensity)")
    out_pts, out_box, _, _, _, _ = run_frames(eng, p, [0, int(p.shape[0])], b, cls, v, [0, n_box], [draws], np.zeros(4, np.float32))
    for src, dst in ((out_box, gt_boxes), (out_pts, points)):
        if dst is None:
            continue
        if isinstance(dst, torch.Tensor):
            dst.copy_(src.reshape(dst.shape))
        else:
            dst[...] = src.cpu().numpy().reshape(dst.shape)


def _step(steps):
    """Draw record of one global function: no noise tries, no permutation."""
    return dict(loc=np.zeros((0, 1, 3)), rot=np.zeros((0, 1)), grot=np.zeros((0, 1)), prm=identity_params(steps), perm=None)


# ---------------------------------------------------------------------------------------------- the reference's functions
def noise_per_object(gt_boxes, points=None, valid_mask=None, rotation_perturb=ROTATION_PERTURB, center_noise_std=CENTER_NOISE_STD,
                     global_random_rot_range=GLOBAL_RANDOM_ROT_RANGE, num_try=NUM_TRY):
    """augmentation.py:177-212 with the noise_per_box_v2_ path (global_random_rot_range > 0.01 deg).  In place."""
    if (rotation_perturb, center_noise_std, global_random_rot_range) != (ROTATION_PERTURB, CENTER_NOISE_STD, GLOBAL_RANDOM_ROT_RANGE):
        raise ValueError("noise_per_object: only the defaults GenericDataset uses are implemented")
    n = int(gt_boxes.shape[0])
    if n > _lib.PP_AUG_MAX_BOXES:
        raise ValueError(f"noise_per_object: {n} boxes exceed PP_AUG_MAX_BOXES {_lib.PP_AUG_MAX_BOXES}")
    loc, rot, grot = draw_noise(n, num_try)
    if n == 0:
        return
    _apply_one(gt_boxes, points, dict(loc=loc, rot=rot, grot=grot, prm=identity_params(ST_MOVE), perm=None), valid_mask)


def random_flip(gt_boxes, points):
    d = _step(ST_FLIP)
    d["prm"][P_FLIP] = draw_flip()
    _apply_one(gt_boxes, points, d)
    return gt_boxes, points


def global_rotation_v2(gt_boxes, points):
    d = _step(ST_ROT)
    d["prm"][P_PITCH:P_YAW + 1] = draw_rotation()
    _apply_one(gt_boxes, points, d)
    return gt_boxes, points


def global_scaling_v2(gt_boxes, points, min_scale=0.85, max_scale=1.15):
    d = _step(ST_SCALE)
    d["prm"][P_SX:P_SZ + 1] = draw_scaling()
    _apply_one(gt_boxes, points, d)
    return gt_boxes, points


def global_translate(gt_boxes, points, noise_translate_std):
    d = _step(ST_TRANS)
    d["prm"][P_TX:P_TZ + 1] = draw_translate(noise_translate_std)
    _apply_one(gt_boxes, points, d)
    return gt_boxes, points
