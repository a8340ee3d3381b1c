#!/usr/bin/env python3
"""Kernel time of PFN training (csrc/pfn_train.hip) at the real shapes -- eight_20cm at 16000 pillars x 15 slots and nuscene at
12000 x 100 -- next to pp_pfn on the same input: HIP events around back-to-back C calls whose arguments are built beforehand, beside
the algorithmic HBM bytes of each call (and those bytes / 8 TB/s, the constant bench.py uses).

    python tools/pfntrain_probe.py [--configs eight_20cm,nuscene] [--reps 20] [--timeout 120]
    rocprofv3 --kernel-trace --stats -d OUT -o pfntrain -- python tools/pfntrain_probe.py --one eight_20cm   (per-kernel split:
                        pfn_stats_kernel, pfn_stats_finish, pfn_train_kernel, scatter_bwd_kernel, pfn_bwd_kernel, pfn_bwd_finish)
Every config runs in a child process of its own under a time limit of its own; the parent never opens the GPU and stops at the
first child that fails.  Note that pp_pfn_train_forward reads the pillar count back (one stream synchronisation per call), which the
event time of back-to-back calls includes.  Prints one JSON line per config."""
import argparse
import ctypes
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BS = 8.0e12
PILLARS = {"eight_20cm": 16000, "nuscene": 12000}


def one(name, reps):
    import numpy as np
    import torch
    pkg = importlib.import_module("3d_object_detection_amd")
    pkg.install()
    synth = importlib.import_module("3d_object_detection_amd.synth")
    engm = importlib.import_module("3d_object_detection_amd.engine")
    cfg = synth.load_config(name)
    cfg["device"] = torch.device("cuda:0")
    eng = engm.Engine(cfg)
    sd = {k: np.asarray(v, np.float32) for k, v in synth.seeded_state_dict(0).items()}
    eng.load_state_dict(sd)
    P, T = PILLARS[name], eng.T
    assert P <= eng.max_voxels
    gx, gy = int(eng.grid_size[0]), int(eng.grid_size[1])
    rng = np.random.default_rng(0)
    cells = rng.choice(gx * gy, P, replace=False)
    coors = np.stack([cells // gy, cells % gy, np.zeros(P, np.int64)], 1).astype(np.int32)
    npts = np.minimum(rng.geometric(0.25, P), T).astype(np.int32)  # most pillars hold a few points, as in a real cloud
    u = rng.random((P, T, 4))
    vs, off = eng.voxel_size, eng.offset
    vox = np.stack([(coors[:, None, 0] + u[:, :, 0]) * vs[0] + off[0], (coors[:, None, 1] + u[:, :, 1]) * vs[1] + off[1], u[:, :, 2] * 3.0 - 2.0,
                    u[:, :, 3]], -1)
    vox = (vox * (np.arange(T)[None, :] < npts[:, None])[:, :, None]).astype(np.float32)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    vox, coors, npts = d(vox), d(coors), d(npts)
    w, gamma, beta = (d(sd[k]) for k in eng.PFN_KEYS)
    rm, rv = (d(sd[k]) for k in eng.PFN_STAT_KEYS)
    num = eng.num_tensor(P)
    feat, arg, stats = eng.pfn_train_forward(vox, coors, npts, num, w, gamma, beta)
    dcanvas = torch.randn((1, 64, gx, gy), device="cuda")
    dfeat = eng.scatter_backward(dcanvas, coors, num)
    dw, dg, db = eng.pfn_backward(vox, coors, npts, num, w, gamma, stats, feat, arg, dfeat)
    out_feat = torch.empty_like(feat)
    lib, ctx, st = eng.lib, eng.ctx, torch.cuda.current_stream().cuda_stream
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def timed(fn):
        assert fn() == 0
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / reps

    calls = {
        "pfn": (lambda: lib.pp_pfn(ctx, ptr(vox), ptr(coors), ptr(npts), ptr(num), ptr(out_feat), st), P * (16 * T + 256)),
        "pfn_train_forward": (lambda: lib.pp_pfn_train_forward(ctx, ptr(vox), ptr(coors), ptr(npts), ptr(num), ptr(w), ptr(gamma), ptr(beta), ptr(feat),
                                                               ptr(arg), ptr(stats), st), P * (2 * 16 * T + 256 + 64)),
        "scatter_backward": (lambda: lib.pp_scatter_backward(ctx, ptr(dcanvas), ptr(coors), ptr(num), ptr(dfeat), st), P * (64 * 4 + 256)),
        "pfn_backward": (lambda: lib.pp_pfn_backward(ctx, ptr(vox), ptr(coors), ptr(npts), ptr(num), ptr(w), ptr(gamma), ptr(stats), ptr(feat), ptr(arg),
                                                     ptr(dfeat), ptr(dw), ptr(dg), ptr(db), st), P * (16 * T + 256 + 256 + 64)),
        "update_pfn_weights": (lambda: lib.pp_update_pfn_weights(ctx, ptr(w), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), st), 5 * 1024),
    }
    out = {"config": name, "pillars": P, "slots": T, "reps": reps}
    for rnd in range(2):  # the second round is the one reported
        for k, (fn, nbytes) in calls.items():
            ms = timed(fn)
            out[k] = {"ms": round(ms, 5), "hbm_bytes": int(nbytes), "hbm_floor_ms": round(nbytes / HBM_BS * 1e3, 5)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="eight_20cm,nuscene")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per config (a child process each)")
    ap.add_argument("--one", help="run this config in this process")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.reps)
    for name in a.configs.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, "--reps", str(a.reps)], timeout=a.timeout)
        if r.returncode != 0:
            sys.exit(f"pfntrain_probe: {name} ended with status {r.returncode}; nothing more is started")


if __name__ == "__main__":
    main()
