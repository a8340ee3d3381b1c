#!/usr/bin/env python3
"""Time of ground-truth database sampling (csrc/gt_sample.hip, framework/gt_sampler.py): HIP events around back-to-back Engine calls
whose arguments are uploaded beforehand, for 32 eight_20cm frames of 20 000 points with 20 boxes + 35 candidates each and 32 frames
of 120 000 points with 60 boxes + 35 candidates; GenericDataset.get_batch (device mode) on a temporary data_root with and without
config["gt_sampler"], the two in alternating windows; build_database per frame.

    python tools/gtsample_probe.py [--frames 32] [--reps 20] [--windows 4]
    rocprofv3 --kernel-trace --stats -d OUT -o gtsample -- python tools/gtsample_probe.py      (per-kernel split)
Prints one JSON line.  paste floor: 16 B in and 16 B out per scene point + 32 B per pasted point, at the 6.29 TB/s a float4 copy
achieves on this chip."""
import argparse
import importlib
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE = 6.29e12
N_CAND = 35


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def frames(synth, nb, n_points, n_boxes, seed):
    """clouds with 60 points inside every box, boxes on a ring around the sensor, kept apart"""
    rng = np.random.default_rng(seed)
    clouds, boxes = [], []
    for f in range(nb):
        ang = np.linspace(0, 2 * np.pi, n_boxes, endpoint=False) + rng.uniform(0, 0.05)
        rad = rng.uniform(8, 60, n_boxes)
        b = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.full(n_boxes, -1.0), np.full(n_boxes, 4.5), np.full(n_boxes, 1.9),
                      np.full(n_boxes, 1.6), rng.uniform(-3, 3, n_boxes)], 1).astype(np.float32)
        u = rng.uniform(-0.45, 0.45, (n_boxes, 60, 3))
        c, s = np.cos(b[:, 6])[:, None], np.sin(b[:, 6])[:, None]
        lx, ly, lz = u[..., 0] * b[:, 3:4], u[..., 1] * b[:, 4:5], u[..., 2] * b[:, 5:6]
        ins = np.stack([lx * c - ly * s + b[:, 0:1], lx * s + ly * c + b[:, 1:2], lz + b[:, 2:3], rng.uniform(0, 1, lx.shape)], -1)
        cloud = synth.lidar_cloud("eight_20cm", seed=seed + f, n_points=n_points - 60 * n_boxes)
        clouds.append(np.concatenate([cloud, ins.reshape(-1, 4).astype(np.float32)]))
        boxes.append(b)
    return clouds, boxes


def write_root(root, clouds, boxes):
    infos = []
    for i, (c, b) in enumerate(zip(clouds, boxes)):
        c.astype(np.float32).tofile(os.path.join(root, f"{i:06d}.bin"))
        infos.append({"velodyne_path": f"{i:06d}.bin", "image_idx": i, "img_shape": np.array([375, 1242], np.int32), "calib/R0_rect": np.eye(4),
                      "calib/Tr_velo_to_cam": np.eye(4), "calib/P2": np.eye(4),
                      "annos": {"name": np.array(["car"] * len(b), dtype="<U10"), "location": b[:, :3].copy(), "dimensions": b[:, 3:6].copy(),
                                "rotation_y": b[:, 6].copy(), "num_points": np.full(len(b), 60, np.int32),
                                "difficulty": np.zeros(len(b), np.int32)}})
    with open(os.path.join(root, "infos.pkl"), "wb") as fh:
        pickle.dump(infos, fh)


def case(cfg, eng, mods, nb, n_points, n_boxes, reps, windows, seed):
    synth, gts, dsm = mods
    clouds, boxes = frames(synth, nb, n_points, n_boxes, seed)
    dev = eng.device
    with tempfile.TemporaryDirectory() as root:
        write_root(root, clouds, boxes)
        cfg = dict(cfg, data_root=root)
        t0 = time.perf_counter()
        db = gts.build_database(cfg, ["infos.pkl"])
        torch.cuda.synchronize()
        build_ms = (time.perf_counter() - t0) * 1e3 / nb
        db.save(os.path.join(root, "db.npz"))
        # the kernels, one by one
        rng = np.random.default_rng(seed)
        po = list(range(0, (nb + 1) * n_points, n_points))
        bo = list(range(0, (nb + 1) * n_boxes, n_boxes))
        co = list(range(0, (nb + 1) * N_CAND, N_CAND))
        pts = torch.from_numpy(np.concatenate(clouds)).to(dev)
        B = torch.from_numpy(np.concatenate(boxes)).to(dev)
        rows = np.concatenate([rng.choice(len(db), N_CAND, replace=False) for _ in range(nb)])
        ci = torch.from_numpy(rows.astype(np.int32)).to(dev)
        dbp, dbo, dbb = db.device(eng)
        cand = dbb[ci.long()]
        counts = eng.gt_count(pts, po, B, bo)
        obj_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counts.long(), 0)])
        T = int(obj_off[-1])
        acc = eng.gt_select(B, bo, cand, co)
        out_n, blk = eng.gt_paste_count(pts, po, cand, ci, acc, co, dbp, dbo, True)
        n_h = out_n.cpu().numpy()
        oo = np.concatenate([[0], np.cumsum(n_h)]).tolist()
        out = torch.empty((oo[-1], 4), dtype=torch.float32, device=dev)
        k = np.full((nb, len(db.detect_class)), 0, np.int32)
        k[:, 0] = N_CAND
        r = dict(frames=nb, points=n_points, boxes=n_boxes, candidates=N_CAND, db_objects=len(db), accepted_per_frame=round(float(acc.sum()) / nb, 1),
                 build_database_ms_per_frame=round(build_ms, 3),
                 count_ms=round(timed(lambda: eng.gt_count(pts, po, B, bo), reps), 4),
                 extract_ms=round(timed(lambda: eng.gt_extract(pts, po, B, bo, obj_off, T), reps), 4),
                 draw_ms=round(timed(lambda: eng.gt_draw(7, 0, list(range(nb)), db.class_off.tolist(), k), reps), 4),
                 select_ms=round(timed(lambda: eng.gt_select(B, bo, cand, co), reps), 4),
                 paste_count_ms=round(timed(lambda: eng.gt_paste_count(pts, po, cand, ci, acc, co, dbp, dbo, True), reps), 4),
                 paste_ms=round(timed(lambda: eng.gt_paste(pts, po, cand, ci, acc, co, dbp, dbo, blk, oo, True, out=out), reps), 4))
        pasted = int((db.offsets[rows + 1] - db.offsets[rows])[acc.cpu().numpy().astype(bool)].sum())
        floor = (nb * n_points + pasted + int(n_h.sum())) * 16 / COPY_RATE * 1e3  # scene rows in, object rows in, output rows out
        r["paste_floor_ms"] = round(floor, 4)
        r["paste_vs_floor"] = round(r["paste_ms"] / floor, 2)
        # the loader, with and without the sampler, in alternating windows
        vg = importlib.import_module("3d_object_detection_amd.framework.voxel_generator").VoxelGenerator(cfg)
        aa = importlib.import_module("3d_object_detection_amd.framework.anchor_assigner").AnchorAssigner(cfg)
        plain = dsm.GenericDataset(cfg, ["infos.pkl"], vg, aa, rng="device", seed=1)
        scfg = dict(cfg, gt_sampler={"database": "db.npz", "sample_groups": {db.detect_class[0]: n_boxes + N_CAND}, "remove_points": True})
        sampled = dsm.GenericDataset(scfg, ["infos.pkl"], vg, aa, rng="device", seed=1)
        idx = list(range(nb))
        t = {"plain": [], "sampled": []}
        for _ in range(windows):
            for name, ds in (("plain", plain), ("sampled", sampled)):
                t[name].append(timed(lambda: ds.get_batch(idx), max(2, reps // 5)))
        r["get_batch_ms"] = round(float(np.median(t["plain"])), 3)
        r["get_batch_sampled_ms"] = round(float(np.median(t["sampled"])), 3)
        r["get_batch_windows"] = {k_: [round(v, 2) for v in vs] for k_, vs in t.items()}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=4)
    a = ap.parse_args()
    synth = importlib.import_module("3d_object_detection_amd.synth")
    eng_mod = importlib.import_module("3d_object_detection_amd.engine")
    gts = importlib.import_module("3d_object_detection_amd.framework.gt_sampler")
    dsm = importlib.import_module("3d_object_detection_amd.framework.dataset")
    cfg = synth.load_config("eight_20cm")
    cfg["device"] = torch.device("cuda:0")
    cfg["max_batch"] = a.frames
    cfg["max_points"] = 1 << 17
    eng = eng_mod.engine_for(cfg)
    eng.load_state_dict(synth.seeded_state_dict(0))
    out = dict(eight_20cm=case(cfg, eng, (synth, gts, dsm), a.frames, 20000, 20, a.reps, a.windows, 1000),
               large=case(cfg, eng, (synth, gts, dsm), a.frames, 120000, 60, a.reps, a.windows, 2000))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
