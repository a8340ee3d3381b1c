#!/usr/bin/env python3
"""Kernel time of the training-target side (csrc/assign.hip) for one 32-frame eight_20cm batch, against the inference pass it
follows: HIP events around back-to-back C calls whose arguments are built and checked beforehand (no host work between launches).

    python tools/assign_probe.py [--frames 32] [--reps 20] [--boxes 20]
    rocprofv3 --kernel-trace --stats -d OUT -o assign -- python tools/assign_probe.py     (per-kernel split: k_gt_prep, k_gmax,
                                                                                             k_assign, k_loss_mem, k_loss_fused, k_loss_final)
Prints one JSON line: ms per call of infer_batch, pp_assign_targets, pp_target_loss, pp_batch_loss, and the HBM bytes each
call must move at least (their floors at 6.3 TB/s achievable)."""
import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--boxes", type=int, default=20)
    a = ap.parse_args()
    synth = importlib.import_module("3d_object_detection_amd.synth")
    engine = importlib.import_module("3d_object_detection_amd.engine")
    nb = a.frames
    cfg = synth.load_config("eight_20cm")
    cfg["device"] = torch.device("cuda:0")
    cfg["max_batch"] = nb
    eng = engine.engine_for(cfg)
    eng.load_state_dict(synth.seeded_state_dict(0, cls_bias=-3.0))
    d = eng.device
    rng = np.random.default_rng(0)
    clouds = [synth.lidar_cloud("eight_20cm", seed=200 + i) for i in range(nb)]
    boxes, classes, off = [], [], [0]
    for c in clouds:
        p = c[rng.integers(0, c.shape[0], a.boxes)]
        boxes.append(np.concatenate([p[:, :2], np.full((a.boxes, 1), -1.0), rng.uniform([0.7, 0.6, 1.5], [5, 2.2, 2.0], (a.boxes, 3)),
                                     rng.uniform(-np.pi, np.pi, (a.boxes, 1))], 1).astype(np.float32))
        classes.append(rng.integers(1, 4, a.boxes).astype(np.int32))
        off.append(off[-1] + a.boxes)
    box = torch.from_numpy(np.concatenate(boxes)).to(d)
    cls = torch.from_numpy(np.concatenate(classes)).to(d)
    offh = (ctypes.c_int32 * (nb + 1))(*off)
    pts = [torch.from_numpy(c).to(d) for c in clouds]
    det, cnt = eng.infer_batch(pts)
    masks = torch.stack([eng.fetch(f, "mask") for f in range(nb)])
    c = torch.stack([eng.fetch(f, "cls") for f in range(nb)])
    b = torch.stack([eng.fetch(f, "box") for f in range(nb)])
    dr = torch.stack([eng.fetch(f, "dir") for f in range(nb)])
    A = eng.A
    lab = torch.empty((nb, A), dtype=torch.int32, device=d)
    tgt = torch.empty((nb, A, 7), dtype=torch.float32, device=d)
    ow = torch.empty((nb, A), dtype=torch.float32, device=d)
    dirt = torch.empty((nb, A), dtype=torch.int32, device=d)
    terms = torch.empty((nb, 21), dtype=torch.float64, device=d)
    lib, ctx, st = eng.lib, eng.ctx, torch.cuda.current_stream().cuda_stream
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def timed(fn):
        rc = fn()
        assert rc in (0, None), rc
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.reps

    out = {"frames": nb, "anchors": A, "boxes_per_frame": a.boxes, "inside_fraction": float(masks.float().mean())}
    out["infer_batch_ms"] = timed(lambda: eng.infer_batch(pts, det, cnt) and None)
    out["assign_targets_ms"] = timed(lambda: lib.pp_assign_targets(ctx, P(masks), P(box), P(cls), offh, nb, P(lab), P(tgt), P(ow), P(dirt), st))
    npos = float((lab > 0).sum())
    out["target_loss_ms"] = timed(lambda: lib.pp_target_loss(ctx, P(c), P(b), P(dr), P(lab), P(tgt), P(dirt), nb, P(terms), st))
    eng.infer_batch(pts, det, cnt)
    out["batch_loss_ms"] = timed(lambda: lib.pp_batch_loss(ctx, P(box), P(cls), offh, nb, P(terms), st))
    # least HBM traffic: assign reads the mask (1 B) and writes 40 B per anchor; the loss kernels read logit, label and direction
    # target (12 B; the fused one: logit + mask, 5 B) per anchor, and box / target / dir rows of the positives only
    n = nb * A
    floors = {"assign_targets": 41 * n, "target_loss": 12 * n + 72 * npos, "batch_loss": 5 * n + 44 * npos}
    for k, v in floors.items():
        out[k + "_floor_ms"] = v / 6.3e12 * 1e3
    out["positives"] = npos
    print(json.dumps(out))


if __name__ == "__main__":
    main()
