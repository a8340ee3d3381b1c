#!/usr/bin/env python3
"""Kernel time of the batch-statistics BatchNorm backward primitives next to their frozen-statistics siblings, in the scheme of
bntrain_probe.py: pp_unit_backward_bn / pp_down_backward_bn / pp_neck_backward_bn against pp_unit_backward_affine /
pp_down_backward_affine / pp_neck_backward_affine at the three level shapes of eight_20cm, at nb = 1 and 8, with du / dx and the two
sums, all on the BatchNorm context of one process.  HIP events around back-to-back C calls whose arguments are built beforehand; a
figure is the median of `--windows` windows of `--reps` calls each, the calls taking turns window by window, so a drift of the clocks
reaches all of them; every row carries its windows' min and max.

Also: the lock-step forward pp_backbone_train_taps_bn over 8 frames against 8 per-frame passes of pp_backbone_train_taps, and whole
training steps at nb = 8 on the BatchNorm network under train(scope="rpn", bn_stats="moving") next to bn_stats="frozen" (forward,
head, loss, backward, SGD step, upload of the sixteen convolutions, three upsamplers and the fold).

    python tools/bnbatch_probe.py [--frames 1,8] [--reps 10] [--windows 5] [--no-step]

Prints one JSON line."""
import argparse
import ctypes
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,8")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="skip the forward and whole-step lines")
    a = ap.parse_args()
    frames = [int(v) for v in a.frames.split(",")]
    pkg = importlib.import_module("3d_object_detection_amd")
    pkg.install()
    synth = importlib.import_module("3d_object_detection_amd.synth")
    export = importlib.import_module("3d_object_detection_amd.networks.pointpillars8_export")
    vgm = importlib.import_module("3d_object_detection_amd.framework.voxel_generator")
    lgm = importlib.import_module("3d_object_detection_amd.framework.loss_generator")
    cfg = synth.load_config("eight_20cm")
    cfg["device"] = torch.device("cuda:0")
    cfg["max_batch"] = max(frames + [8])
    vgm.VoxelGenerator(cfg)
    net = export.PointPillars(cfg)
    net.load_state_dict(synth.seeded_state_dict(0, norm="batch", cls_bias=-3.0))
    eng = net._eng
    d, A, H, W = eng.device, eng.A, eng.H, eng.W
    lib, st = eng.lib, torch.cuda.current_stream().cuda_stream
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    gen = torch.Generator(device=d).manual_seed(0)

    def timed(fn, reps=a.reps):
        rc = fn()
        assert rc in (0, None), rc
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / reps

    out = {"map": [H, W], "reps": a.reps, "windows": a.windows, "rows": []}
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    rnd = lambda *s: torch.randn(s, device=d, generator=gen)  # noqa: E731
    for nb in frames:
        y, dy320 = torch.relu(rnd(nb, 320, H, W)), rnd(nb, 320, H, W)
        calls = {}
        for b in (2, 1, 0):
            C, cin, h, w = 64 << b, eng.DOWN_PAIRS[b][0], H >> b, W >> b
            wsh = eng.neck_shapes(b)[1]
            wu, w0, wn = rnd(C, C, 3, 3) * 0.05, rnd(C, cin, 3, 3) * 0.05, rnd(*wsh) * 0.05
            x, z, dy = rnd(nb, cin, 2 * h, 2 * w), rnd(nb, C, h, w), rnd(nb, C, h, w)
            sc, sh = torch.rand(C, device=d, generator=gen) + 0.5, rnd(C) * 0.1
            mean, var = z.mean((0, 2, 3)).contiguous(), z.var((0, 2, 3), unbiased=False).contiguous()
            dwu, dw0, dwn, du, dx, dxn = (torch.empty_like(t) for t in (wu, w0, wn, z, x, z))
            ds, dh = torch.empty(C, dtype=torch.float64, device=d), torch.empty(C, dtype=torch.float64, device=d)
            t = dict(C=C, cin=cin, h=h, w=w, b=b, wu=wu, w0=w0, wn=wn, x=x, z=z, dy=dy, sc=sc, sh=sh, mean=mean, var=var, dwu=dwu, dw0=dw0,
                     dwn=dwn, du=du, dx=dx, dxn=dxn, ds=ds, dh=dh)
            calls[b] = dict(
                keep=t, ms={},
                unit=lambda t=t: lib.pp_unit_backward_affine(eng.ctx, t["C"], t["h"], t["w"], ptr(t["z"]), ptr(t["wu"]), ptr(t["sc"]), ptr(t["sh"]),
                                                             ptr(t["dy"]), ptr(t["dy"]), nb, ptr(t["dwu"]), ptr(t["du"]), ptr(t["ds"]), ptr(t["dh"]), st),
                unit_bn=lambda t=t: lib.pp_unit_backward_bn(eng.ctx, t["C"], t["h"], t["w"], ptr(t["z"]), ptr(t["wu"]), ptr(t["sc"]), ptr(t["sh"]),
                                                            ptr(t["mean"]), ptr(t["var"]), ptr(t["dy"]), ptr(t["dy"]), nb, ptr(t["dwu"]), ptr(t["du"]),
                                                            ptr(t["ds"]), ptr(t["dh"]), 0, st),
                down=lambda t=t: lib.pp_down_backward_affine(eng.ctx, t["cin"], t["C"], 2 * t["h"], 2 * t["w"], ptr(t["x"]), ptr(t["w0"]), ptr(t["z"]),
                                                             ptr(t["sc"]), ptr(t["sh"]), ptr(t["dy"]), nb, ptr(t["dw0"]), ptr(t["dx"]), ptr(t["ds"]),
                                                             ptr(t["dh"]), st),
                down_bn=lambda t=t: lib.pp_down_backward_bn(eng.ctx, t["cin"], t["C"], 2 * t["h"], 2 * t["w"], ptr(t["x"]), ptr(t["w0"]), ptr(t["z"]),
                                                            ptr(t["sc"]), ptr(t["sh"]), ptr(t["mean"]), ptr(t["var"]), ptr(t["dy"]), nb, ptr(t["dw0"]),
                                                            ptr(t["dx"]), ptr(t["ds"]), ptr(t["dh"]), 0, st),
                neck=lambda t=t: lib.pp_neck_backward_affine(eng.ctx, t["b"], ptr(t["z"]), ptr(t["wn"]), ptr(t["sc"]), ptr(t["sh"]), ptr(y), ptr(dy320),
                                                             nb, ptr(t["dwn"]), ptr(t["dxn"]), ptr(t["ds"]), ptr(t["dh"]), st),
                neck_bn=lambda t=t: lib.pp_neck_backward_bn(eng.ctx, t["b"], ptr(t["z"]), ptr(t["wn"]), ptr(t["sc"]), ptr(t["sh"]), ptr(t["mean"]),
                                                            ptr(t["var"]), ptr(y), ptr(dy320), nb, ptr(t["dwn"]), ptr(t["dxn"]), ptr(t["ds"]),
                                                            ptr(t["dh"]), 0, st))
        kinds = ("unit", "unit_bn", "down", "down_bn", "neck", "neck_bn")
        for win in range(a.windows + 1):  # the first round warms up (workspaces grow, clocks rise) and is dropped
            for b in (2, 1, 0):
                for k in kinds:
                    t = timed(calls[b][k])
                    if win:
                        calls[b]["ms"].setdefault(k, []).append(t)
        for b in (0, 1, 2):
            for k in kinds[::2]:
                i, f = calls[b]["ms"][k], calls[b]["ms"][k + "_bn"]
                out["rows"].append(dict(frames=nb, call=k + "_backward", level=b, affine_ms=med(i), affine_min=min(i), affine_max=max(i),
                                        bn_ms=med(f), bn_min=min(f), bn_max=max(f), bn_over_affine=med(f) / med(i)))
        del calls, y, dy320
        torch.cuda.empty_cache()
    if not a.no_step:
        nb = 8
        canv = []
        for i in range(nb):
            pts = torch.from_numpy(synth.lidar_cloud("eight_20cm", seed=300 + i)).to(d)
            vox, coors, npts, num = eng.voxelize(pts)
            canv.append(eng.scatter(eng.pfn(vox, coors, npts, num), coors, num))
        canv = torch.cat(canv)
        params = {k: p.detach() for attr in ("_rpn", "_down", "_block", "_neck") for k, p in getattr(net, attr).items()}
        fw = {"lockstep": [], "per_frame": []}
        for win in range(a.windows + 1):
            for k, fn in (("lockstep", lambda: eng.backbone_train_taps_bn(canv, params) and None),
                          ("per_frame", lambda: [eng.backbone_train_taps(c) for c in canv] and None)):
                t = timed(fn, reps=3)
                if win:
                    fw[k].append(t)
        out["forward_nb8"] = {k: dict(ms=med(v), min=min(v), max=max(v)) for k, v in fw.items()}
        torch.cuda.empty_cache()
        r = torch.rand((nb, A), device=d, generator=gen)
        ex = {"labels": torch.where(r < 0.002, 1, torch.where(r < 0.3, 0, -1)).to(torch.int32),
              "bbox_targets": torch.randn((nb, A, 7), device=d, generator=gen) * 0.3,
              "dir_targets": (torch.rand((nb, A), device=d, generator=gen) < 0.5).to(torch.int32)}
        lg = lgm.LossGenerator(cfg)

        def step(opt):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            rpn = net.rpn_train(canv)
            ev[1].record()
            loss = lg.generate(net.heads(rpn), ex)["loss"]
            ev[2].record()
            opt.zero_grad()
            loss.backward()
            opt.step()
            net._sync_head()
            net._sync_neck()
            ev[3].record()
            torch.cuda.synchronize()
            parts = {k: ev[i].elapsed_time(ev[i + 1]) for k, i in (("backbone_forward_ms", 0), ("head_and_loss_ms", 1), ("backward_step_upload_ms", 2))}
            return dict(parts, total_ms=sum(parts.values()))

        for stats in ("frozen", "moving"):
            net.train(scope="rpn", bn_stats=stats)
            opt = torch.optim.SGD(net.parameters(), lr=1e-3)
            step(opt)
            out[f"step_nb8_rpn_{stats}"] = [step(opt) for _ in range(3)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
