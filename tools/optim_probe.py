#!/usr/bin/env python3
"""Time of the optimizer part of a training step on the 28 tensors of net.train(scope="all") for eight_20cm (4 826 010 elements), with
random gradients, four variants in one process:

    a  framework.optim.clip_grad_norm_ + Adam.step()               (norm, scale, Adam: three passes)
    b  framework.optim.Adam.step(clip_norm=10.0)                    (norm, Adam reading the coefficient on the device)
    c  torch.nn.utils.clip_grad_norm_ + torch.optim.Adam.step()     (torch's default implementation)
    d  the same with torch.optim.Adam(fused=True)

HIP events around `--reps` back-to-back calls; a figure is the median of `--windows` such windows after a warm-up round that is dropped,
and the variants take turns window by window, so a drift of the clocks reaches all of them; every row carries its windows' min and max.
The events see what the stream sees: where the host cannot issue a variant's launches as fast as the device retires them, the figure is
the host's.  `floor_ms` is one Adam pass at the HBM peak bench.py uses for its stage rooflines: 28 B per element (p, g, m, v read, p, m,
v written) / 8 TB/s; `over_floor` = time / floor.  `adam_kernel` and `norm_kernels` are the C calls alone with their argument arrays
built beforehand.  With --step: whole scope="all" steps at nb = 8 (eight synthetic clouds: forward, loss, backward, clip + Adam) with
torch's optimizer and with this one, alternated three times.  Prints one JSON line.

    python tools/optim_probe.py [--reps 20] [--windows 7] [--step]"""
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
HBM_PEAK_GBS = 8000.0  # bench.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--step", action="store_true", help="also time whole scope='all' steps at nb = 8")
    a = ap.parse_args()
    pkg = importlib.import_module("3d_object_detection_amd")
    pkg.install()
    synth = importlib.import_module("3d_object_detection_amd.synth")
    shared = importlib.import_module("3d_object_detection_amd.networks.pointpillars8_shared")
    vgm = importlib.import_module("3d_object_detection_amd.framework.voxel_generator")
    lgm = importlib.import_module("3d_object_detection_amd.framework.loss_generator")
    utils = importlib.import_module("3d_object_detection_amd.framework.utils")
    optim = importlib.import_module("3d_object_detection_amd.framework.optim")
    cfg = synth.load_config("eight_20cm")
    cfg["device"] = torch.device("cuda:0")
    cfg["max_batch"] = 8
    vgen = vgm.VoxelGenerator(cfg)
    net = shared.PointPillars(cfg)
    net.load_state_dict(synth.seeded_state_dict(0, cls_bias=-3.0))
    net.train(scope="all")
    eng = net._eng
    d = eng.device
    gen = torch.Generator(device=d).manual_seed(0)
    shapes = [tuple(p.shape) for p in net.parameters()]
    n_el = sum(int(np.prod(s)) for s in shapes)
    floor_ms = 28.0 * n_el / (HBM_PEAK_GBS * 1e9) * 1e3

    def fresh_params():
        ps = [torch.nn.Parameter(p.detach().clone()) for p in net.parameters()]
        for p in ps:
            p.grad = torch.randn(p.shape, device=d, generator=gen) * 1e-2
        return ps

    def variant(kind):
        ps = fresh_params()
        if kind in "ab":
            opt = optim.Adam(ps, lr=1e-3)
            if kind == "a":
                def call():
                    optim.clip_grad_norm_(ps, 10.0)
                    opt.step()
            else:
                def call():
                    opt.step(clip_norm=10.0)
        else:
            opt = torch.optim.Adam(ps, lr=1e-3, fused=kind == "d")

            def call():
                torch.nn.utils.clip_grad_norm_(ps, 10.0)
                opt.step()
        return call

    # the C calls alone
    ps = fresh_params()
    ms_, vs_ = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    lens = (ctypes.c_int64 * len(ps))(*[p.numel() for p in ps])
    ap_, ag_, am_, av_ = arr(ps), arr([p.grad for p in ps]), arr(ms_), arr(vs_)
    out2 = torch.tensor([0.0, 1.0], device=d)
    lib, ctx, st = eng.lib, eng.ctx, torch.cuda.current_stream().cuda_stream
    po = ctypes.c_void_p(out2.data_ptr())
    po1 = ctypes.c_void_p(out2.data_ptr() + 4)
    calls = {"a": variant("a"), "b": variant("b"), "c": variant("c"), "d": variant("d"),
             "adam_kernel": lambda: lib.pp_adam_step(ctx, ap_, ag_, am_, av_, lens, len(ps), 7, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, po1, st),
             "norm_kernels": lambda: lib.pp_grad_norm(ctx, ag_, lens, len(ps), 10.0, po, st)}

    def timed(fn):
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.reps

    ms = {k: [] for k in calls}
    for win in range(a.windows + 1):  # the first round warms up and is dropped
        for k, fn in calls.items():
            t = timed(fn)
            if win:
                ms[k].append(t)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    out = {"tensors": len(shapes), "elements": n_el, "reps": a.reps, "windows": a.windows, "floor_ms": floor_ms,
           "rows": {k: dict(ms=med(v), ms_min=min(v), ms_max=max(v), over_floor=med(v) / floor_ms) for k, v in ms.items()}}
    r = out["rows"]
    best_torch = min(r["c"]["ms"], r["d"]["ms"])
    out["b_minus_best_torch_ms"] = r["b"]["ms"] - best_torch
    out["b_spread_ms"] = r["b"]["ms_max"] - r["b"]["ms_min"]
    out["b_not_slower"] = bool(r["b"]["ms"] - best_torch <= out["b_spread_ms"])
    if a.step:
        frames = []
        for i in range(8):
            v, c, n = vgen.generate(synth.lidar_cloud("eight_20cm", seed=300 + i))
            frames.append(dict(voxels=v, coordinates=c, num_points_per_voxel=n))
        example = utils.example_convert_to_torch(utils.merge_second_batch(frames))
        A = eng.A
        rr = torch.rand((8, A), device=d, generator=gen)
        ex = {"labels": torch.where(rr < 0.002, 1, torch.where(rr < 0.3, 0, -1)).to(torch.int32),
              "bbox_targets": torch.randn((8, A, 7), device=d, generator=gen) * 0.3,
              "dir_targets": (torch.rand((8, A), device=d, generator=gen) < 0.5).to(torch.int32)}
        lg = lgm.LossGenerator(cfg)
        sd = net.state_dict()

        def step(opt, ours):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            loss = lg.generate(net(example), ex)["loss"]
            opt.zero_grad()
            loss.backward()
            ev[1].record()
            if ours:
                opt.step(clip_norm=10.0)
            else:
                torch.nn.utils.clip_grad_norm_(net.parameters(), 10.0)
                opt.step()
            ev[2].record()
            torch.cuda.synchronize()
            parts = dict(forward_loss_backward_ms=ev[0].elapsed_time(ev[1]), optimizer_ms=ev[1].elapsed_time(ev[2]))
            return dict(parts, total_ms=sum(parts.values()))

        for rnd in range(3):
            for name, ours in (("torch", False), ("device", True)):
                net.load_state_dict(sd)
                net.train(scope="all")
                opt = (optim.Adam if ours else torch.optim.Adam)(net.parameters(), lr=1e-3)
                step(opt, ours)
                out.setdefault("step_nb8_all_" + name, []).append(step(opt, ours))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
