#!/usr/bin/env python3
"""Generate tests/golden/augment_small.npz and augment_dataset.npz by RUNNING THE REFERENCE (needs the reference tree; ~1 min).

    python tests/golden/make_augment_goldens.py

Reuses make_goldens.install_shims (numba as identity decorators).  Per frame (small synthetic clouds trimmed around the boxes):
np.random.seed(seed), then the reference's noise_per_object, random_flip, global_rotation_v2, global_scaling_v2 and
global_translate exactly as GenericDataset.__getitem__ calls them (dataset.py:126-133), then its range filter and limit_period
(:136-143) and the shuffle (:146).  The stored stream state is the next np.random.random() after the frame.  The selected tries come
from the reference's noise_per_box_v2_ on the same draws.

augment_dataset.npz: the reference's own GenericDataset(...).__getitem__ on a temporary data_root (a synthetic info pickle with a
<U10 name array, one .bin cloud) for augm=True, augm=False and training=False, with a non-detect-class annotation first and box
rotations outside (-pi, pi], so that limit_period does work on the augm=False path.

The generator asserts:
  - every collision decision and every point-face sign of the frame lies at least MARGIN from its threshold (tests/augment_ref.py
    records them), so float32 rounding differences (BLAS FMAs in the reference's matmuls) cannot flip one;
  - no selected try depends on box_collision_test's containment branch, which numba runs and plain Python does not;
  - the covered cases exist: early tries rejected, a box with no successful try, an invalid box first (dataset.py:126-127), no
    boxes, boxes outside every range edge after the chain.
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import REF, ROOT, install_shims, save  # noqa: E402

MARGIN = 2e-5  # float32 corners of 80 m scenes carry ~5e-6 of rounding; 1e-4 left no seed for frame 0
RANGE = np.array([-80.0, -80.0, 80.0, 80.0], np.float32)
# frame seeds (np.random.seed before the frame); a seed whose frame violates MARGIN is replaced and the new one recorded here
SEEDS = [11, 12, 13, 14]


def frame_inputs(f, synth):
    """(boxes f32[N,7], valid bool[N], points f32[M,4]) of frame f."""
    rng = np.random.default_rng(100 + f)
    if f == 0:  # overlapping boxes: early tries rejected; two boxes overlapping by half: box 1 finds no try
        boxes = [[10.0, 5.0, -1.0, 4.5, 1.9, 1.6, 0.3], [12.2, 5.4, -1.0, 4.5, 1.9, 1.6, 0.35], [13.5, 3.0, -1.0, 4.0, 1.8, 1.5, 1.2],
                 [-20.0, -8.0, -0.8, 0.8, 0.7, 1.75, -0.7], [-20.0, -9.2, -0.8, 1.8, 0.7, 1.7, 2.5]]
        valid = [True, True, True, True, True]
    elif f == 1:  # quirk 1: the first annotation is not a detect class, so box 0 keeps valid False
        boxes = [[30.0, -30.0, -1.0, 4.5, 1.9, 1.6, -1.0], [31.0, -26.5, -1.0, 4.6, 2.0, 1.7, 2.9], [5.0, 40.0, -1.0, 1.8, 0.7, 1.7, 0.1]]
        valid = [False, True, True]
    elif f == 2:  # no boxes
        boxes, valid = np.zeros((0, 7)), []
    else:  # boxes pushed across the range edges by the chain
        boxes = [[79.5, 0.0, -1.0, 4.5, 1.9, 1.6, 0.0], [-81.5, 10.0, -1.0, 4.5, 1.9, 1.6, 1.4], [0.0, 81.0, -1.0, 4.5, 1.9, 1.6, 0.7],
                 [20.0, -82.5, -1.0, 4.5, 1.9, 1.6, -2.2], [40.0, 40.0, -1.0, 4.5, 1.9, 1.6, 3.0]]
        valid = [True] * 5
    boxes = np.asarray(boxes, np.float32).reshape(-1, 7)
    cloud = synth.lidar_cloud("eight_20cm", seed=200 + f, n_points=3000)
    pts = [cloud]
    for b in boxes:  # points inside and around each box
        u = rng.uniform(-0.6, 0.6, size=(80, 3)).astype(np.float32)
        c, s = np.cos(b[6]), np.sin(b[6])
        lx, ly, lz = u[:, 0] * b[3], u[:, 1] * b[4], u[:, 2] * b[5]
        p = np.stack([lx * c - ly * s + b[0], lx * s + ly * c + b[1], lz + b[2], rng.uniform(0, 1, 80)], axis=1)
        pts.append(p.astype(np.float32))
    return boxes, np.asarray(valid, bool), np.concatenate(pts).astype(np.float32)


def frame_margin(R, boxes, valid, pts, seed):
    n = boxes.shape[0]
    np.random.seed(seed)
    loc = np.random.normal(scale=np.array([0.15] * 3, np.float32), size=[n, 100, 3])
    rot = np.random.uniform(-5.0 / 180 * np.pi, 5.0 / 180 * np.pi, size=[n, 100])
    grot = np.random.uniform(-2.0 / 180 * np.pi, 2.0 / 180 * np.pi, size=[n, 100])
    margins = []
    R.noise_select(boxes, valid, loc, rot, grot, True, margins)
    R.membership(pts[:, :3], boxes, valid, margins)
    return min(margins) if margins else np.inf


def main():
    install_shims()
    sys.path.insert(0, REF)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import importlib
    synth = importlib.import_module("3d_object_detection_amd.synth")
    import augment_ref as R
    from framework import augmentation as ragm
    from framework import box_np_ops

    out = dict(range=RANGE, margin=MARGIN)
    cases = dict(rejected=False, none=False, quirk1=False, empty=False, dropped=False)
    for f, seed in enumerate(SEEDS):
        boxes, valid, pts = frame_inputs(f, synth)
        # trim points that lie within the margin of a face plane of some box (their membership would rest on rounding)
        near = np.zeros(pts.shape[0], bool)
        for j in range(boxes.shape[0]):
            pl = R.face_planes(boxes[j])
            sg = ((pts[:, 0:1] * pl[:, 0] + pts[:, 1:2] * pl[:, 1]) + pts[:, 2:3] * pl[:, 2]) + pl[:, 3]
            near |= (np.abs(sg) <= 2 * MARGIN).any(axis=1)
        pts = np.ascontiguousarray(pts[~near])
        for _ in range(10):
            if frame_margin(R, boxes, valid, pts, seed) > MARGIN:
                break
            print(f"frame {f}: seed {seed} violates the margin; SEEDS must name another")
            seed += 100
        SEEDS[f] = seed
        n = boxes.shape[0]
        # the reference, as __getitem__ runs it
        np.random.seed(seed)
        b = boxes.copy()
        p = pts.copy()
        ragm.noise_per_object(b, p, valid)
        after_noise = (b.copy(), p.copy())
        b, p = ragm.random_flip(b, p)
        b, p = ragm.global_rotation_v2(b, p)
        b, p = ragm.global_scaling_v2(b, p, min_scale=0.95, max_scale=1.05)
        b, p = ragm.global_translate(b, p, noise_translate_std=[0.25, 0.25, 0.25])
        keep = np.asarray(box_np_ops.filter_gt_box_outside_range(b, RANGE), bool) if n else np.zeros(0, bool)
        b = b[keep]
        b[:, 6] = box_np_ops.limit_period(b[:, 6], offset=0.5, period=2 * np.pi)
        p_unshuffled = p.copy()
        np.random.shuffle(p)
        nxt = np.random.random()
        # the same draws again: selected tries from the reference's noise_per_box_v2_, global parameters, permutation
        np.random.seed(seed)
        loc = np.random.normal(scale=np.array([0.15] * 3, np.float32), size=[n, 100, 3])
        rot = np.random.uniform(-5.0 / 180 * np.pi, 5.0 / 180 * np.pi, size=[n, 100])
        grot = np.random.uniform(-2.0 / 180 * np.pi, 2.0 / 180 * np.pi, size=[n, 100])
        sel = ragm.noise_per_box_v2_(boxes[:, [0, 1, 3, 4, 6]], valid, loc.copy(), rot.copy(), grot.copy()) if n else np.zeros(0, np.int64)
        flip = np.random.random() > 0.5
        pitch, roll, yaw = (np.random.uniform(-a, a) / 180 * np.pi for a in (4, 2, 30))
        sc = [np.random.uniform(0.9, 1.1), np.random.uniform(0.9, 1.1), np.random.uniform(0.95, 1.05)]
        tr = [float(np.random.normal(0, 0.25, 1)[0]) for _ in range(3)]
        perm = np.random.permutation(pts.shape[0])
        assert np.random.random() == nxt, "the redrawn stream does not end where the reference's frame ended"
        assert np.array_equal(p_unshuffled[perm], p), "points[perm] differs from the shuffled array"
        # margins and the containment branch, on the oracle
        margins, contained = [], []
        s_num, _, _ = R.noise_select(boxes, valid, loc, rot, grot, True, margins, contained)
        s_py, _, _ = R.noise_select(boxes, valid, loc, rot, grot, False)
        assert np.array_equal(s_num, sel) and np.array_equal(s_py, sel), f"frame {f}: oracle tries {s_num} / {s_py}, reference {sel}"
        R.membership(pts[:, :3], boxes, valid, margins)
        mmin = min(margins) if margins else np.inf
        assert mmin > MARGIN, f"frame {f} seed {seed}: a decision lies {mmin:.2e} from its threshold"
        cases["rejected"] |= bool((sel > 0).any())
        cases["none"] |= bool((sel[valid] == -1).any()) if n else False
        cases["quirk1"] |= bool(n and not valid[0])
        cases["empty"] |= n == 0
        cases["dropped"] |= bool(n and not keep.all())
        prm = np.array([63, float(flip), pitch, roll, yaw, *sc, *tr, 0, 0, 0, 0, 0], np.float64)
        out.update({f"boxes_{f}": boxes, f"valid_{f}": valid, f"points_{f}": pts, f"sel_{f}": sel.astype(np.int32), f"prm_{f}": prm,
                    f"perm_{f}": perm.astype(np.int32), f"next_{f}": nxt, f"noise_boxes_{f}": after_noise[0],
                    f"noise_points_{f}": after_noise[1], f"out_boxes_{f}": b, f"keep_{f}": keep, f"out_points_{f}": p,
                    f"margin_{f}": mmin, f"contained_{f}": len(contained)})
        print(f"frame {f}: seed {seed}, {n} boxes, sel {sel.tolist()}, keep {keep.tolist()}, margin {mmin:.2e}, "
              f"{len(contained)} containment tests true")
    assert all(cases.values()), cases
    out["seeds"] = np.array(SEEDS, np.int64)
    save("augment_small", **out)


DS_SEEDS = {"augm": 21, "noaugm": 22, "eval": 23}
DS_NAMES = np.array(["tree", "car", "person", "truck", "bicycle"], dtype="<U10")  # 'tree' is no detect class: quirk 1


def dataset_inputs(R, synth):
    """The annotation boxes (camera-free lidar boxes, as the info stores them) and the trimmed cloud of the dataset frames."""
    boxes = np.array([[-30.0, 20.0, -1.0, 4.5, 1.9, 1.6, 0.5], [30.0, -30.0, -1.0, 4.5, 1.9, 1.6, -3.9],
                      [5.0, 40.0, -1.0, 0.8, 0.7, 1.75, 4.2], [-12.0, -25.0, -0.8, 7.5, 2.6, 2.9, 3.6],
                      [15.0, 12.0, -0.9, 1.8, 0.7, 1.7, -3.4]], np.float32)
    rng = np.random.default_rng(300)
    pts = [synth.lidar_cloud("eight_20cm", seed=301, n_points=3000)]
    for b in boxes:
        u = rng.uniform(-0.6, 0.6, size=(80, 3)).astype(np.float32)
        c, s_ = np.cos(b[6]), np.sin(b[6])
        lx, ly, lz = u[:, 0] * b[3], u[:, 1] * b[4], u[:, 2] * b[5]
        pts.append(np.stack([lx * c - ly * s_ + b[0], lx * s_ + ly * c + b[1], lz + b[2], rng.uniform(0, 1, 80)], axis=1).astype(np.float32))
    pts = np.concatenate(pts).astype(np.float32)
    near = np.zeros(pts.shape[0], bool)
    for j in range(boxes.shape[0]):
        pl = R.face_planes(boxes[j])
        sg = ((pts[:, 0:1] * pl[:, 0] + pts[:, 1:2] * pl[:, 1]) + pts[:, 2:3] * pl[:, 2]) + pl[:, 3]
        near |= (np.abs(sg) <= 2 * MARGIN).any(axis=1)
    return boxes, np.ascontiguousarray(pts[~near])


def write_data_root(root, boxes, pts):
    """The synthetic info pickle and cloud the tests rebuild from the stored arrays (tests/test_augment_gpu.py does the same)."""
    import pickle
    pts.astype(np.float32).tofile(os.path.join(root, "000000.bin"))
    info = {"velodyne_path": "000000.bin", "image_idx": 0, "img_shape": np.array([375, 1242], np.int32),
            "calib/R0_rect": np.eye(4), "calib/Tr_velo_to_cam": np.eye(4), "calib/P2": np.eye(4),
            "annos": {"name": DS_NAMES.copy(), "location": boxes[:, :3].copy(), "dimensions": boxes[:, 3:6].copy(),
                      "rotation_y": boxes[:, 6].copy(), "num_points": np.full(len(boxes), 10, np.int32),
                      "difficulty": np.arange(len(boxes), dtype=np.int32)}}
    with open(os.path.join(root, "infos.pkl"), "wb") as fh:
        pickle.dump([info], fh)


def dataset_goldens():
    import importlib
    import tempfile
    synth = importlib.import_module("3d_object_detection_amd.synth")
    import augment_ref as R
    from framework.voxel_generator import VoxelGenerator
    from framework.anchor_assigner import AnchorAssigner
    from framework.dataset import GenericDataset
    boxes, pts = dataset_inputs(R, synth)
    out = dict(boxes=boxes, points=pts, names=DS_NAMES)
    with tempfile.TemporaryDirectory() as root:
        write_data_root(root, boxes, pts)
        for case, seed in DS_SEEDS.items():
            cfg = synth.load_config("eight_20cm")
            cfg["data_root"] = root
            cfg["create_mask_gpu"] = 0
            vg = VoxelGenerator(cfg)
            aa = AnchorAssigner(cfg)
            ds = GenericDataset(cfg, ["infos.pkl"], vg, aa, training=case != "eval", augm=case == "augm")
            # the margins of this frame's decisions under this seed (class-filtered boxes, the quirk-1 valid mask)
            info = ds.infos[0]
            m = np.array([n in ds.detect_class for n in info["annos"]["name"]])
            fb = np.concatenate([info["annos"]["location"][m], info["annos"]["dimensions"][m], info["annos"]["rotation_y"][m][:, None]],
                                1).astype(np.float32)
            valid = np.array([n in ds.augm_class for n in info["annos"]["name"]])[:len(fb)]
            if case == "augm":
                mg = frame_margin(R, fb, valid, pts, seed)
                assert mg > MARGIN, f"dataset seed {seed}: margin {mg:.2e}"
                assert not valid[0] and m[0] == False  # noqa: E712  quirk 1 is exercised
            np.random.seed(seed)
            ex = ds[0]
            nxt = np.random.random()
            out[f"{case}_next"] = nxt
            out[f"{case}_coordinates"] = ex["coordinates"]
            out[f"{case}_npts"] = ex["num_points_per_voxel"]
            out[f"{case}_points"] = ex["points"]
            if case != "eval":
                a = ex["annos"]
                if case == "noaugm":
                    assert (np.abs(fb[:, 6]) > np.pi).any(), "no rotation outside (-pi, pi]: limit_period would be idle"
                out.update({f"{case}_gt_boxes": a["gt_boxes"], f"{case}_gt_classes": a["gt_classes"], f"{case}_gt_names": a["gt_names"],
                            f"{case}_difficulty": a["difficulty"], f"{case}_pos": np.nonzero(ex["labels"] > 0)[0].astype(np.int32),
                            f"{case}_labels_sha": __import__("make_goldens").sha(ex["labels"].astype(np.int32))})
            else:
                assert "annos" not in ex and "labels" not in ex
            print(f"dataset {case}: seed {seed}, {ex['coordinates'].shape[0]} pillars, "
                  f"{0 if case == 'eval' else len(ex['annos']['gt_boxes'])} boxes")
    save("augment_dataset", **out)


if __name__ == "__main__":
    main()
    dataset_goldens()
