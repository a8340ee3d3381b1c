"""GPU side of the training-input augmentation (csrc/augment.hip): the kernels against the reference goldens, the reference-named
functions in place, GenericDataset end to end, get_batch against stacked __getitem__, and the host checks."""
import importlib
import os
import pickle
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import augment_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
agm = importlib.import_module("3d_object_detection_amd.framework.augmentation")
dsm = importlib.import_module("3d_object_detection_amd.framework.dataset")
synth = importlib.import_module("3d_object_detection_amd.synth")
G = np.load(os.path.join(HERE, "golden", "augment_small.npz"))
FRAMES = list(range(len(G["seeds"])))


def _close(a, b, rel=2e-6):
    d = np.abs(a.astype(np.float64) - b) / np.maximum(1.0, np.abs(b.astype(np.float64)))
    return d.size == 0 or d.max() <= rel


def _run(frames):
    eng = agm._engine()
    dev = eng.device
    draws, pts, boxes, valid = [], [], [], []
    for f in frames:
        np.random.seed(int(G["seeds"][f]))
        draws.append(agm.draw_frame(G[f"points_{f}"].shape[0], G[f"boxes_{f}"].shape[0], True, True))
        pts.append(G[f"points_{f}"]); boxes.append(G[f"boxes_{f}"]); valid.append(G[f"valid_{f}"])
    po = np.concatenate([[0], np.cumsum([p.shape[0] for p in pts])]).tolist()
    bo = np.concatenate([[0], np.cumsum([b.shape[0] for b in boxes])]).tolist()
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    B = t(np.concatenate(boxes).reshape(-1, 7), np.float32)
    cls = torch.arange(B.shape[0], dtype=torch.int32, device=dev)
    out = agm.run_frames(eng, t(np.concatenate(pts), np.float32), po, B, cls, t(np.concatenate(valid), np.uint8), bo, draws, G["range"])
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out], po, bo


def test_kernels_against_reference_goldens():
    (p, b, c, keep, kept, sel), po, bo = _run(FRAMES)
    worst = 0.0
    for z, f in enumerate(FRAMES):
        assert np.array_equal(sel[bo[z]:bo[z + 1]], G[f"sel_{f}"]), f"frame {f}: selected tries"
        assert np.array_equal(keep[bo[z]:bo[z + 1]].astype(bool), G[f"keep_{f}"]), f"frame {f}: kept boxes"
        k = int(kept[z])
        assert k == int(G[f"keep_{f}"].sum())
        assert np.array_equal(c[bo[z]:bo[z] + k], np.nonzero(G[f"keep_{f}"])[0] + bo[z])  # in order
        assert _close(b[bo[z]:bo[z] + k], G[f"out_boxes_{f}"]), f"frame {f}: boxes"
        assert _close(p[po[z]:po[z + 1]], G[f"out_points_{f}"]), f"frame {f}: points"
        assert np.array_equal(p[po[z]:po[z + 1], 3], G[f"out_points_{f}"][:, 3])
        for a, r in ((b[bo[z]:bo[z] + k], G[f"out_boxes_{f}"]), (p[po[z]:po[z + 1]], G[f"out_points_{f}"])):
            if r.size:
                worst = max(worst, float((np.abs(a.astype(np.float64) - r) / np.maximum(1.0, np.abs(r))).max()))
    print(f"max relative deviation from the reference: {worst:.3e}")


def test_batch_equals_single_frames():
    (p, b, c, keep, kept, sel), po, bo = _run(FRAMES)
    for z, f in enumerate(FRAMES):
        (p1, b1, _, k1, n1, s1), _, _ = _run([f])
        assert np.array_equal(p[po[z]:po[z + 1]], p1) and np.array_equal(s1, sel[bo[z]:bo[z + 1]])
        assert np.array_equal(b[bo[z]:bo[z] + int(n1[0])], b1[:int(n1[0])])


@pytest.mark.parametrize("f", [0, 1])
def test_noise_per_object_in_place(f):
    boxes, valid, pts = G[f"boxes_{f}"].copy(), G[f"valid_{f}"], G[f"points_{f}"].copy()
    np.random.seed(int(G["seeds"][f]))
    agm.noise_per_object(boxes, pts, valid)
    assert _close(boxes, G[f"noise_boxes_{f}"]) and _close(pts, G[f"noise_points_{f}"])
    # device tensors in place give the same values
    tb = torch.from_numpy(G[f"boxes_{f}"].copy()).cuda()
    tp = torch.from_numpy(G[f"points_{f}"].copy()).cuda()
    np.random.seed(int(G["seeds"][f]))
    agm.noise_per_object(tb, tp, valid)
    assert np.array_equal(tb.cpu().numpy(), boxes) and np.array_equal(tp.cpu().numpy(), pts)


def test_global_functions_match_oracle():
    f = 0
    b, p = G[f"boxes_{f}"].copy(), G[f"points_{f}"].copy()
    np.random.seed(5)
    agm.random_flip(b, p)
    agm.global_rotation_v2(b, p)
    agm.global_scaling_v2(b, p)
    agm.global_translate(b, p, [0.25, 0.25, 0.25])
    np.random.seed(5)
    prm = agm.identity_params(agm.ST_FLIP | agm.ST_ROT | agm.ST_SCALE | agm.ST_TRANS)
    prm[1] = agm.draw_flip(); prm[2:5] = agm.draw_rotation(); prm[5:8] = agm.draw_scaling(); prm[8:11] = agm.draw_translate()
    z = np.zeros((b.shape[0], 3)), np.zeros(b.shape[0])
    rb, _ = R.boxes_chain(G[f"boxes_{f}"], G[f"valid_{f}"], z[0], z[1], prm, G["range"])
    rp = R.points_chain(G[f"points_{f}"], G[f"boxes_{f}"], G[f"valid_{f}"], z[0], z[1], prm)
    assert _close(b, rb) and _close(p, rp)


def _data_root(tmp_path, n=3):
    cfg = synth.load_config("eight_20cm")
    infos = []
    for i in range(n):
        f = FRAMES[i % 2]
        pts = G[f"points_{f}"]
        name = f"{i:06d}.bin"
        pts.astype(np.float32).tofile(tmp_path / name)
        bx = G[f"boxes_{f}"]
        names = np.array(["car", "person", "truck", "tree"][:len(bx)] + ["car"] * max(0, len(bx) - 4), dtype="<U10")
        if i == 1:
            names[0] = "tree"  # quirk 1: a non-detect-class annotation first
        infos.append({"velodyne_path": name, "image_idx": i, "img_shape": np.array([375, 1242], np.int32),
                      "calib/R0_rect": np.eye(4), "calib/Tr_velo_to_cam": np.eye(4), "calib/P2": np.eye(4),
                      "annos": {"name": names, "location": bx[:, :3].copy(), "dimensions": bx[:, 3:6].copy(), "rotation_y": bx[:, 6].copy(),
                                "num_points": np.full(len(bx), 10, np.int32), "difficulty": np.zeros(len(bx), np.int32)}})
    with open(tmp_path / "infos.pkl", "wb") as fh:
        pickle.dump(infos, fh)
    cfg["data_root"] = str(tmp_path)
    cfg["device"] = torch.device("cuda:0")
    cfg["max_batch"] = 4
    return cfg


def _dataset(cfg, **kw):
    vg = importlib.import_module("3d_object_detection_amd.framework.voxel_generator").VoxelGenerator(cfg)
    aa = importlib.import_module("3d_object_detection_amd.framework.anchor_assigner").AnchorAssigner(cfg)
    return dsm.GenericDataset(cfg, ["infos.pkl"], vg, aa, **kw)


def test_getitem_end_to_end(tmp_path):
    cfg = _data_root(tmp_path)
    ds = _dataset(cfg)
    assert len(ds) == 3
    for i in range(3):
        np.random.seed(40 + i)
        ex = ds[i]
        info = ds.infos[i]
        a = info["annos"]
        m = np.array([n in ds.detect_class for n in a["name"]])
        boxes = np.concatenate([a["location"][m], a["dimensions"][m], a["rotation_y"][m][:, None]], 1).astype(np.float32)
        valid = np.array([n in ds.augm_class for n in a["name"]])[:len(boxes)]
        pts = G[f"points_{FRAMES[i % 2]}"]
        np.random.seed(40 + i)
        d = agm.draw_frame(pts.shape[0], len(boxes), True, True)
        sel, sl, sr = R.noise_select(boxes, valid, d["loc"], d["rot"], d["grot"])
        rb, keep = R.boxes_chain(boxes, valid, sl, sr, d["prm"], ds.detection_range[[0, 1, 3, 4]])
        rp = R.points_chain(pts, boxes, valid, sl, sr, d["prm"], d["perm"])
        assert np.array_equal(ex["annos"]["gt_names"], a["name"][m][keep])
        assert _close(ex["annos"]["gt_boxes"], rb[keep]) and _close(ex["points"], rp)
        assert ex["labels"].shape == ex["anchors_mask"].shape and ex["bbox_targets"].shape[1] == 7
        _downstream_against_oracles(ds, ex)


def _downstream_against_oracles(ds, ex):
    """The GPU's own augmented cloud through the CPU oracles (oracle/c_oracle.py voxeliser and mask, tests/assign_ref.py): voxels,
    coordinates, mask and labels exact."""
    from oracle import c_oracle as C
    from oracle import pp_oracle as O
    import assign_ref
    cfg = synth.load_config("eight_20cm")
    st = O.voxel_setup(cfg)
    vo, co, no = C.points_to_voxels(ex["points"], st["voxel_size"], st["offset"], st["grid_size"], cfg["max_voxels"], cfg["max_num_points"])
    assert np.array_equal(co, ex["coordinates"]) and np.array_equal(no, ex["num_points_per_voxel"]) and np.array_equal(vo, ex["voxels"])
    eng = ds._engine()
    mask = C.create_mask(co, st["grid_size"], eng.rects_np).astype(bool)
    assert np.array_equal(mask, ex["anchors_mask"])
    names = list(eng.class_masks)
    tm = [eng.class_table[n].get("matched_threshold", 0.6) for n in names]
    tu = [eng.class_table[n].get("unmatched_threshold", 0.45) for n in names]
    ref = assign_ref.assign_frame(eng.anchors_np, eng.anchors_bv, list(eng.class_masks.values()), tm, tu, ex["annos"]["gt_boxes"],
                                  ex["annos"]["gt_classes"], mask)
    assert np.array_equal(ref["labels"], ex["labels"])
    # the assignment contract (tests/test_assign_gpu.py): x / y / z / r codes bit-exact, the log codes within 2 ulp
    t, rt = ex["bbox_targets"], ref["bbox_targets"]
    assert np.array_equal(t[:, [0, 1, 2, 6]], rt[:, [0, 1, 2, 6]])
    np.testing.assert_array_max_ulp(t[:, 3:6], rt[:, 3:6], maxulp=2)
    assert np.array_equal(ref["dir_targets"], ex["dir_targets"])


D = np.load(os.path.join(HERE, "golden", "augment_dataset.npz"))


def _reference_root(tmp_path):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    info = {"velodyne_path": "000000.bin", "image_idx": 0, "img_shape": np.array([375, 1242], np.int32), "calib/R0_rect": np.eye(4),
            "calib/Tr_velo_to_cam": np.eye(4), "calib/P2": np.eye(4),
            "annos": {"name": D["names"].copy(), "location": D["boxes"][:, :3].copy(), "dimensions": D["boxes"][:, 3:6].copy(),
                      "rotation_y": D["boxes"][:, 6].copy(), "num_points": np.full(len(D["boxes"]), 10, np.int32),
                      "difficulty": np.arange(len(D["boxes"]), dtype=np.int32)}}
    D["points"].astype(np.float32).tofile(tmp_path / "000000.bin")
    with open(tmp_path / "infos.pkl", "wb") as fh:
        pickle.dump([info], fh)
    cfg = synth.load_config("eight_20cm")
    cfg["data_root"] = str(tmp_path)
    cfg["device"] = torch.device("cuda:0")
    return cfg


def _pillars_near_edges(pts, cfg, eps=1e-4):
    """BEV cells of the points that lie within eps of a voxel edge (in x or y)."""
    from oracle import pp_oracle as O
    st = O.voxel_setup(cfg)
    q = (pts[:, :2].astype(np.float64) - st["offset"][:2]) / st["voxel_size"][:2]
    near = (np.abs(q - np.round(q)) * st["voxel_size"][:2] < eps).any(axis=1)
    return {tuple(c) for c in np.floor(q[near]).astype(np.int64)[:, ::-1]} | {tuple(c) for c in np.round(q[near]).astype(np.int64)[:, ::-1]}


@pytest.mark.parametrize("case", ["augm", "noaugm", "eval"])
def test_getitem_against_reference_dataset(tmp_path, case):
    """GenericDataset[0] against the reference's own __getitem__ on the same data_root and seed (tests/golden/augment_dataset.npz)."""
    cfg = _reference_root(tmp_path)
    seeds = {"augm": 21, "noaugm": 22, "eval": 23}
    ds = _dataset(cfg, training=case != "eval", augm=case == "augm")
    np.random.seed(seeds[case])
    ex = ds[0]
    assert np.random.random() == float(D[f"{case}_next"])
    if case == "augm":
        assert _close(ex["points"], D["augm_points"])
    else:
        assert np.array_equal(ex["points"], D[f"{case}_points"])
    if case != "eval":
        a = ex["annos"]
        assert np.array_equal(a["gt_names"], D[f"{case}_gt_names"]) and np.array_equal(a["gt_classes"], D[f"{case}_gt_classes"])
        assert np.array_equal(a["difficulty"], D[f"{case}_difficulty"])
        if case == "augm":
            assert _close(a["gt_boxes"], D["augm_gt_boxes"])
        else:  # range filter + limit_period of rotations outside (-pi, pi]: bit for bit
            assert np.array_equal(a["gt_boxes"], D["noaugm_gt_boxes"])
            assert (np.abs(D["boxes"][:, 6]) > np.pi).any() and (np.abs(a["gt_boxes"][:, 6]) <= np.pi).all()
            assert np.array_equal(np.nonzero(ex["labels"] > 0)[0], D["noaugm_pos"])
        _downstream_against_oracles(ds, ex)
    got = {tuple(c[1:]) for c in ex["coordinates"]}
    ref = {tuple(c[1:]) for c in D[f"{case}_coordinates"]}
    if case == "augm":  # pillar differences only where a point lies within 1e-4 of a voxel edge
        assert (got ^ ref) <= (_pillars_near_edges(ex["points"], cfg) | _pillars_near_edges(D["augm_points"], cfg))
    else:
        assert np.array_equal(ex["coordinates"], D[f"{case}_coordinates"]) and np.array_equal(ex["num_points_per_voxel"], D[f"{case}_npts"])


def test_containment_collides_on_gpu():
    """Quirk 2 on the device: a small box inside a large one; every try of either keeps the containment, no edge crosses.  numba's
    semantics (the product's) reject every try, plain Python would accept try 0."""
    eng = agm._engine()
    boxes = np.array([[20.0, 5.0, -1.0, 1.0, 0.8, 1.5, 0.4], [20.0, 5.0, -1.0, 10.0, 6.0, 2.0, 0.1]], np.float32)
    valid = np.ones(2, bool)
    np.random.seed(77)
    loc, rot, grot = agm.draw_noise(2)
    ref, _, _ = R.noise_select(boxes, valid, loc, rot, grot, containment=True)
    py, _, _ = R.noise_select(boxes, valid, loc, rot, grot, containment=False)
    assert ref.tolist() == [-1, -1] and py[0] == 0
    d = eng.device
    sel, _, _ = eng.augment_noise(torch.from_numpy(boxes).to(d), torch.ones(2, dtype=torch.uint8, device=d), torch.from_numpy(loc).to(d),
                                  torch.from_numpy(rot).to(d), torch.from_numpy(grot).to(d), [0, 2])
    assert sel.cpu().numpy().tolist() == ref.tolist()


# ---------------------------------------------------------------------------------------------- device random mode
def _dev_frames(n_frames, n_pts=500, n_boxes=2):
    eng = agm._engine()
    rng = np.random.default_rng(5)
    pts, boxes = [], []
    for f in range(n_frames):
        pts.append(np.concatenate([rng.uniform(-40, 40, (n_pts, 3)), rng.uniform(0, 1, (n_pts, 1))], 1).astype(np.float32))
        b = np.array([[10.0 + 20 * k, -5.0 + f, -1.0, 4.5, 1.9, 1.6, 0.3 * k] for k in range(n_boxes)], np.float32)
        boxes.append(b)
    return eng, pts, boxes


def _dev_run(eng, pts, boxes, samples, seed=3, epoch=0, draws=None):
    dev = eng.device
    po = np.concatenate([[0], np.cumsum([p.shape[0] for p in pts])]).tolist()
    bo = np.concatenate([[0], np.cumsum([b.shape[0] for b in boxes])]).tolist()
    B = torch.from_numpy(np.concatenate(boxes)).to(dev)
    cls = torch.ones(B.shape[0], dtype=torch.int32, device=dev)
    v = torch.ones(B.shape[0], dtype=torch.uint8, device=dev)
    if draws is None:
        draws = agm.draw_device(eng, seed, epoch, samples, bo)
    out = agm.run_frames(eng, torch.from_numpy(np.concatenate(pts)).to(dev), po, B, cls, v, bo, draws, np.array([-80, -80, 80, 80], np.float32))
    return [o.cpu().numpy() for o in out], po, bo, draws


def test_device_mode_deterministic_and_batch_independent():
    eng, pts, boxes = _dev_frames(5)
    a, po, bo, _ = _dev_run(eng, pts, boxes, [10, 11, 12, 13, 14])
    b, _, _, _ = _dev_run(eng, pts, boxes, [10, 11, 12, 13, 14])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for f in (0, 3):  # frame f alone and inside another batch composition
        c, _, _, _ = _dev_run(eng, [pts[f]], [boxes[f]], [10 + f])
        assert np.array_equal(c[0], a[0][po[f]:po[f + 1]]) and np.array_equal(c[5], a[5][bo[f]:bo[f + 1]])
        assert np.array_equal(c[1][:int(c[4][0])], a[1][bo[f]:bo[f] + int(a[4][f])])
    d, _, _, _ = _dev_run(eng, pts, boxes, [10, 11, 12, 13, 14], epoch=1)
    assert not np.array_equal(d[0], a[0])  # another epoch draws afresh


@pytest.mark.parametrize("n", [0, 1, 2, 1000, 1024, 1025, 120000])
def test_device_permutation_is_bijection(n):
    eng = agm._engine()
    pts = [np.zeros((n, 4), np.float32), np.zeros((7, 4), np.float32)]
    po = [0, n, n + 7]
    d = agm.draw_device(eng, 9, 0, [4, 5], [0, 0, 0])
    rec = agm.export_device_draws(eng, d, po)
    assert np.array_equal(np.sort(rec[0]["perm"]), np.arange(n)) and np.array_equal(np.sort(rec[1]["perm"]), np.arange(7))
    if n > 100:
        assert (rec[0]["perm"] != np.arange(n)).mean() > 0.9


def test_device_export_through_numpy_path_bit_identical():
    eng, pts, boxes = _dev_frames(4)
    a, po, bo, d = _dev_run(eng, pts, boxes, [1, 2, 3, 4])
    rec = agm.export_device_draws(eng, d, po)
    assert all(r["perm"] is not None and not int(r["prm"][0]) & agm.ST_PERM for r in rec)
    b, _, _, _ = _dev_run(eng, pts, boxes, None, draws=rec)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def _ks(x, cdf):
    x = np.sort(x)
    n = x.size
    F = cdf(x)
    return max(float(np.max(np.arange(1, n + 1) / n - F)), float(np.max(F - np.arange(n) / n)))


def test_device_draw_distributions():
    """About 2000 frames (one box each): ranges, KS statistics of the uniforms and normals, flip rate, first permutation element."""
    import math
    eng = agm._engine()
    nf = 2048
    prm, loc, rot, grot, first = [], [], [], [], []
    for f0 in range(0, nf, 64):
        d = agm.draw_device(eng, 123, 0, list(range(f0, f0 + 64)), list(range(65)))
        prm.append(d["prm"].cpu().numpy()); loc.append(d["loc"].cpu().numpy()); rot.append(d["rot"].cpu().numpy())
        grot.append(d["grot"].cpu().numpy())
        rec = agm.export_device_draws(eng, d, list(range(0, 65 * 10, 10)))
        first += [int(r["perm"][0]) for r in rec]
    prm, loc, rot, grot = np.concatenate(prm), np.concatenate(loc), np.concatenate(rot), np.concatenate(grot)
    crit = lambda n: 1.63 / math.sqrt(n)  # KS at p = 0.01
    u = lambda lo, hi: (lambda x: np.clip((x - lo) / (hi - lo), 0, 1))
    rp, gp = 5 / 180 * np.pi, 2 / 180 * np.pi
    for x, lo, hi in ((rot.ravel(), -rp, rp), (grot.ravel(), -gp, gp), (prm[:, 5], 0.9, 1.1), (prm[:, 6], 0.9, 1.1), (prm[:, 7], 0.95, 1.05),
                      (prm[:, 2], -4 / 180 * np.pi, 4 / 180 * np.pi), (prm[:, 3], -2 / 180 * np.pi, 2 / 180 * np.pi),
                      (prm[:, 4], -30 / 180 * np.pi, 30 / 180 * np.pi)):
        assert x.min() >= lo and x.max() < hi
        assert _ks(x, u(lo, hi)) < crit(x.size)
    erf = np.vectorize(math.erf)
    ncdf = lambda s: (lambda x: 0.5 * (1 + erf(x / (s * math.sqrt(2)))))
    for x, sd in ((loc[..., 0].ravel()[:60000], float(np.float32(0.15))), (loc[..., 2].ravel()[:60000], float(np.float32(0.15))),
                  (prm[:, 8], 0.25), (prm[:, 10], 0.25)):
        assert _ks(x, ncdf(sd)) < crit(x.size)
    assert abs(prm[:, 1].mean() - 0.5) < 0.05
    counts = np.bincount(first, minlength=10)  # element 0 of a 10-point permutation lands uniformly
    assert counts.min() > 0.6 * nf / 10 and counts.max() < 1.4 * nf / 10


def test_device_mode_dataset(tmp_path):
    cfg = _data_root(tmp_path)
    ds = _dataset(cfg, rng="device", seed=5)
    state = np.random.get_state()[1].copy()
    a = ds[1]
    assert np.array_equal(np.random.get_state()[1], state)  # no host draws
    b = ds.get_batch([0, 1, 2])
    assert np.array_equal(b["points"][b["points_offsets"][1]:b["points_offsets"][2]].cpu().numpy(), a["points"])
    assert np.array_equal(b["labels"][1].cpu().numpy(), a["labels"])
    ds.set_epoch(1)
    assert not np.array_equal(ds[1]["points"], a["points"])
    rec = ds.export_params([1])
    assert sorted(rec[0]["perm"].tolist()) == list(range(a["points"].shape[0]))
    _downstream_against_oracles(ds, a)


def test_get_batch_equals_getitem(tmp_path):
    cfg = _data_root(tmp_path)
    ds = _dataset(cfg)
    np.random.seed(9)
    single = [ds[i] for i in range(3)]
    nxt = np.random.random()
    np.random.seed(9)
    bt = ds.get_batch([0, 1, 2])
    assert np.random.random() == nxt
    assert np.array_equal(bt["voxels"].cpu().numpy(), np.concatenate([e["voxels"] for e in single]))
    co = np.concatenate([np.pad(e["coordinates"], ((0, 0), (0, 1)), constant_values=i) for i, e in enumerate(single)])
    assert np.array_equal(bt["coordinates"].cpu().numpy(), co)
    for k in ("anchors_mask", "labels", "bbox_targets", "dir_targets", "bbox_outside_weights"):
        assert np.array_equal(bt[k].cpu().numpy(), np.stack([e[k] for e in single])), k
    assert np.array_equal(bt["points"].cpu().numpy(), np.concatenate([e["points"] for e in single]))
    for i, e in enumerate(single):
        assert np.array_equal(bt["annos"][i]["gt_boxes"].cpu().numpy(), e["annos"]["gt_boxes"])


def test_modes_without_augmentation(tmp_path):
    cfg = _data_root(tmp_path, 1)
    np.random.seed(1)
    ex = _dataset(cfg, augm=False)[0]
    np.random.seed(1)
    perm = np.random.permutation(G["points_0"].shape[0])
    assert np.array_equal(ex["points"], G["points_0"][perm])
    ev = _dataset(cfg, training=False)[0]
    assert "annos" not in ev and "labels" not in ev and np.array_equal(ev["points"], G["points_0"])
    with pytest.raises(ValueError):
        _dataset(cfg, rng="philox")


def test_bad_inputs_raise():
    eng = agm._engine()
    d = eng.device
    b = torch.zeros((3, 7), device=d)
    v = torch.ones(3, dtype=torch.uint8, device=d)
    loc = torch.zeros((3, 100, 3), dtype=torch.float64, device=d)
    r = torch.zeros((3, 100), dtype=torch.float64, device=d)
    with pytest.raises(ValueError):
        eng.augment_noise(b, v, loc, r, r, [0, 2])  # offsets do not end at G
    with pytest.raises(ValueError):
        eng.augment_noise(b, v, loc, r, r, [0, 3, 2])
    with pytest.raises(TypeError):
        eng.augment_noise(b, v, loc.float(), r, r, [0, 3])
    with pytest.raises(ValueError):
        eng.augment_noise(torch.zeros((300, 7), device=d), torch.ones(300, dtype=torch.uint8, device=d),
                          torch.zeros((300, 1, 3), dtype=torch.float64, device=d), torch.zeros((300, 1), dtype=torch.float64, device=d),
                          torch.zeros((300, 1), dtype=torch.float64, device=d), [0, 300])  # > PP_AUG_MAX_BOXES in a frame
    with pytest.raises(ValueError):
        eng.augment_points(torch.zeros((5, 4), device=d), None, [0, 5], b, v, torch.zeros((3, 3), dtype=torch.float64, device=d),
                           torch.zeros(3, dtype=torch.float64, device=d), torch.zeros((2, 16), dtype=torch.float64, device=d), [0, 3])
