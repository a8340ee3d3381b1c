#!/usr/bin/env python3
"""Kernel time of the backward kernels at every level's shape on eight_20cm: pp_unit_backward at (64, 400 x 400), (128, 200 x 200),
(256, 100 x 100) and pp_down_backward at (64 -> 64, 800 x 800 in), (64 -> 128, 400 x 400 in), (128 -> 256, 200 x 200 in), with du / dx,
at nb = 1 and 8: HIP events around back-to-back C calls whose arguments are built beforehand, next to each call's flop floor -- the
MFMA flops its two products execute / 157.3 TF (the constant bench.py uses).  `over_floor` is time / floor; `vs_block3` is a shape's
over_floor divided by that of the same kernel at block 3's shape in the same run (the target is <= 1.5).  A figure is the median of
`--windows` event windows of `--reps` calls each; the three levels take turns window by window, so a drift of the clocks reaches all of
them, and every row carries its windows' min and max and `vs_block3_worst` = (its slowest window) / (block 3's fastest).

Mixed precision: pp_unit_backward_mp is timed per `--grad-precision` mode (default all three) at the same shapes, the modes taking
turns window by window as well.  A mode's floor is the flops its MFMAs execute over its own padded plane / its rate: fp32 157.3 TF,
bf16 and bf16x3 2.5 PF (the bf16 MFMA roof), bf16x3 executing three MFMAs per product.  `vs_fp32` is median / fp32's median and
`ships` whether the mode's slowest window beats fp32's fastest (the condition for pp_unit_backward_path to hand the shape to it).
pp_down_backward_mp (the same shapes as pp_down_backward) and pp_neck_backward_mp (the three branches of the map) take part in the same
windows, per mode.  Their 16-bit kernels read the fp32 planes, so a mode's floor is the fp32 call's flops x (3 for bf16x3) / 2.5 PF; the
neck's recomputed forward Z = w^T x stays an fp32 product in every mode and is counted at 157.3 TF.  `--only-stages` skips the unit rows.

    python tools/rpntrain_probe.py [--frames 1,8] [--reps 20] [--windows 7] [--grad-precision fp32,bf16x3,bf16]
    rocprofv3 --kernel-trace --stats -d OUT -o rpntrain -- python tools/rpntrain_probe.py --frames 8 --no-step   (per-kernel split)

Also in the same run: pp_update_rpn_weights, pp_backbone_train_taps against pp_backbone_stage_taps, whole fine-tuning steps at nb = 8
under scope "rpn" and "stage3", alternated (per-frame forward, head, loss, backward, SGD step, weight upload), the same step under
scope "rpn" per grad-precision mode, alternated, and the device memory the tensors saved for the backward take per frame under scope
"rpn".  Prints one JSON line."""
import argparse
import ctypes
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MFMA_FS = 157.3e12
BF16_FS = 2.5e15  # the bf16 MFMA roof
MODES = {"fp32": 0, "bf16x3": 1, "bf16": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,8")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--no-step", action="store_true", help="skip the whole-step lines")
    ap.add_argument("--grad-precision", default="fp32,bf16x3,bf16", help="modes of the *_backward_mp entries to time")
    ap.add_argument("--only-stages", action="store_true", help="time pp_down_backward_mp and pp_neck_backward_mp only")
    a = ap.parse_args()
    modes = [m for m in a.grad_precision.split(",") if m]
    assert modes and all(m in MODES for m in modes), a.grad_precision
    frames = [int(v) for v in a.frames.split(",")]
    pkg = importlib.import_module("3d_object_detection_amd")
    pkg.install()
    synth = importlib.import_module("3d_object_detection_amd.synth")
    shared = importlib.import_module("3d_object_detection_amd.networks.pointpillars8_shared")
    vgm = importlib.import_module("3d_object_detection_amd.framework.voxel_generator")
    lgm = importlib.import_module("3d_object_detection_amd.framework.loss_generator")
    cfg = synth.load_config("eight_20cm")
    cfg["device"] = torch.device("cuda:0")
    cfg["max_batch"] = max(frames + [8])
    vgm.VoxelGenerator(cfg)
    net = shared.PointPillars(cfg)
    net.load_state_dict(synth.seeded_state_dict(0, cls_bias=-3.0))
    eng = net._eng
    d, A, H, W = eng.device, eng.A, eng.H, eng.W
    lib, ctx, st = eng.lib, eng.ctx, torch.cuda.current_stream().cuda_stream
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
    for nb in frames:
        calls, rows = {}, {}
        yn = torch.randn((nb, 320, H, W), device=d, generator=gen)  # rpn_out (its sign is the ReLU mask) and dL/d(rpn_out)
        dyn = torch.randn((nb, 320, H, W), device=d, generator=gen)
        for b in (2, 1, 0):  # block 3's shape first: the yardstick of the other two
            C, cin, h, w = 64 << b, eng.DOWN_PAIRS[b][0], H >> b, W >> b
            wu = (torch.randn((C, C, 3, 3), device=d, generator=gen) * 0.05).contiguous()
            w0 = (torch.randn((C, cin, 3, 3), device=d, generator=gen) * 0.05).contiguous()
            x = torch.randn((nb, cin, 2 * h, 2 * w), device=d, generator=gen)
            z = torch.randn((nb, C, h, w), device=d, generator=gen)
            dy = torch.randn((nb, C, h, w), device=d, generator=gen)
            dwu, dw0, du, dx = torch.empty_like(wu), torch.empty_like(w0), torch.empty_like(z), torch.empty_like(x)
            keep = (wu, w0, x, z, dy, dwu, dw0, du, dx)
            unit = lambda C=C, h=h, w=w, z=z, wu=wu, dy=dy, dwu=dwu, du=du: lib.pp_unit_backward(  # noqa: E731
                ctx, C, h, w, ptr(z), ptr(wu), ptr(dy), ptr(dy), nb, ptr(dwu), ptr(du), st)
            mp = {m: (lambda C=C, h=h, w=w, z=z, wu=wu, dy=dy, dwu=dwu, du=du, m=m: lib.pp_unit_backward_mp(  # noqa: E731
                ctx, MODES[m], C, h, w, ptr(z), ptr(wu), ptr(dy), ptr(dy), nb, ptr(dwu), ptr(du), st)) for m in modes}
            for m in modes:
                assert lib.pp_unit_backward_path(ctx, MODES[m], C, h, w) == MODES[m], (m, C, h, w)
            down = lambda C=C, cin=cin, h=h, w=w, x=x, w0=w0, z=z, dy=dy, dw0=dw0, dx=dx: lib.pp_down_backward(  # noqa: E731
                ctx, cin, C, 2 * h, 2 * w, ptr(x), ptr(w0), ptr(z), ptr(dy), nb, ptr(dw0), ptr(dx), st)
            dmp = {m: (lambda C=C, cin=cin, h=h, w=w, x=x, w0=w0, z=z, dy=dy, dw0=dw0, dx=dx, m=m: lib.pp_down_backward_mp(  # noqa: E731
                ctx, MODES[m], cin, C, 2 * h, 2 * w, ptr(x), ptr(w0), ptr(z), ptr(dy), nb, ptr(dw0), ptr(dx), st)) for m in modes}
            xn = torch.randn((nb, C, h, w), device=d, generator=gen)  # the upsampler of level b reads the block output [C][h][w]
            wn = (torch.randn((C, 128 if b else 64, 1 << b, 1 << b), device=d, generator=gen) * 0.05).contiguous()
            dwn, dxn = torch.empty_like(wn), torch.empty_like(xn)
            nmp = {m: (lambda b=b, xn=xn, wn=wn, dwn=dwn, dxn=dxn, m=m: lib.pp_neck_backward_mp(  # noqa: E731
                ctx, MODES[m], b, ptr(xn), ptr(wn), ptr(yn), ptr(dyn), nb, ptr(dwn), ptr(dxn), st)) for m in modes}
            for m in modes:
                assert lib.pp_down_backward_path(ctx, MODES[m], cin, C, 2 * h, 2 * w) == MODES[m], (m, cin, C, h, w)
                assert lib.pp_neck_backward_path(ctx, MODES[m], b) == MODES[m], (m, b)
            keep += (xn, wn, dwn, dxn)
            calls[b] = dict(unit=unit, down=down, keep=keep, ms=dict(unit=[], down=[]), **{"mp_" + m: f for m, f in mp.items()},
                            **{"dmp_" + m: f for m, f in dmp.items()}, **{"nmp_" + m: f for m, f in nmp.items()})
            calls[b]["ms"].update({p + m: [] for m in modes for p in ("mp_", "dmp_", "nmp_")})
            if a.only_stages:
                for k in ["unit", "down"] + ["mp_" + m for m in modes]:
                    del calls[b]["ms"][k]
        for win in range(a.windows + 1):  # the first round warms up (workspaces grow, clocks rise) and is dropped
            for b in (2, 1, 0):
                for k in list(calls[b]["ms"]):
                    t = timed(calls[b][k])
                    if win:
                        calls[b]["ms"][k].append(t)
        for b in (2, 1, 0):
            C, cin, h, w = 64 << b, eng.DOWN_PAIRS[b][0], H >> b, W >> b
            PP = (h + 2) * (w + 2)  # positions a product executes per frame: the zero-haloed plane
            fl = dict(unit=2 * 2.0 * C * 9 * C * PP * nb / MFMA_FS * 1e3, down=2 * 2.0 * C * 9 * cin * PP * nb / MFMA_FS * 1e3)
            sh = dict(unit=[C, h, w], down=[cin, C, 2 * h, 2 * w])
            PP16 = (h + 2) * ((w + 2 + 7) // 8 * 8)  # the 16-bit planes pad the row pitch to a multiple of 8
            for m in modes:
                fl["mp_" + m] = (fl["unit"] if m == "fp32" else (3 if m == "bf16x3" else 1) * 2 * 2.0 * C * 9 * C * PP16 * nb / BF16_FS * 1e3)
                sh["mp_" + m] = [C, h, w]
                mult = (3 if m == "bf16x3" else 1) * MFMA_FS / BF16_FS  # the fp32 call's flops at the mode's rate
                fl["dmp_" + m] = fl["down"] if m == "fp32" else mult * fl["down"]
                sh["dmp_" + m] = sh["down"]
                gemm = 2.0 * C * (128 if b else 64) * h * w * (1 << 2 * b) * nb / MFMA_FS * 1e3  # one Cin x R x p product in fp32
                fl["nmp_" + m] = 3 * gemm if m == "fp32" else gemm + 2 * mult * gemm
                sh["nmp_" + m] = [b, C, h, w]
            rows[b] = {k: dict(shape=sh[k], ms=med(v), ms_min=min(v), ms_max=max(v), floor_ms=fl[k], over_floor=med(v) / fl[k])
                       for k, v in calls[b]["ms"].items()}
        for b in (0, 1, 2):
            for k in () if a.only_stages else ("unit", "down"):
                r, r3 = rows[b][k], rows[2][k]
                out["rows"].append(dict(frames=nb, call=k + "_backward", level=b, **r, vs_block3=r["over_floor"] / r3["over_floor"],
                                        vs_block3_worst=(r["ms_max"] / r["floor_ms"]) / (r3["ms_min"] / r3["floor_ms"])))
        for b in (0, 1, 2):
            for pre, call in (("mp_", "unit_backward_mp"), ("dmp_", "down_backward_mp"), ("nmp_", "neck_backward_mp")):
                f32 = rows[b].get(pre + "fp32")
                for m in modes:
                    if pre + m not in rows[b]:
                        continue
                    r = rows[b][pre + m]
                    extra = dict(vs_fp32=r["ms"] / f32["ms"], ships=r["ms_max"] < f32["ms_min"]) if f32 and m != "fp32" else {}
                    out["rows"].append(dict(frames=nb, call=call, grad_precision=m, level=b, **r, **extra))
        del calls, yn, dyn
        torch.cuda.empty_cache()
    keys = eng.RPN_CONV_KEYS
    every = {**net._rpn, **net._down, **net._block}
    wts = [every[k].detach().clone() for k in keys]
    arr = (ctypes.c_void_p * 16)(*[t.data_ptr() for t in wts])
    out["update_rpn_weights_ms"] = timed(lambda: lib.pp_update_rpn_weights(ctx, arr, st))
    out["conv_tilings"] = [t["tiling"] for t in eng.layer_tilings() if t["kind"] == 0]
    gx, gy = int(eng.grid_size[0]), int(eng.grid_size[1])
    canvas = torch.relu(torch.randn((1, 64, gx, gy), device=d, generator=gen)) * (torch.rand((1, 1, gx, gy), device=d, generator=gen) < 0.03)
    rpn = torch.empty((1, 320, H, W), device=d)
    taps = [torch.empty((1, 64 << b, H >> b, W >> b), device=d) for b in range(3)]
    units = [torch.empty((n, 64 << b, H >> b, W >> b), device=d) for b, n in enumerate(eng.RPN_UNITS)]
    zs = [torch.empty((1, 64 << b, H >> b, W >> b), device=d) for b in range(3)]
    up, zp = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in units]), (ctypes.c_void_p * 3)(*[t.data_ptr() for t in zs])
    for rep in range(2):
        out["backbone_stage_taps_ms"] = timed(lambda: lib.pp_backbone_stage_taps(ctx, ptr(canvas), ptr(rpn), *[ptr(t) for t in taps], ptr(units[2]),
                                                                                 ptr(zs[2]), st))
        out["backbone_train_taps_ms"] = timed(lambda: lib.pp_backbone_train_taps(ctx, ptr(canvas), ptr(rpn), *[ptr(t) for t in taps], up, zp, st))
        out["backbone_ms"] = timed(lambda: lib.pp_backbone(ctx, ptr(canvas), ptr(rpn), st))
    if not a.no_step:
        # whole fine-tuning steps at nb = 8: canvases of 8 clouds (voxelize, PFN, scatter), then per-frame backbone, head, loss,
        # backward, SGD step, weight upload; the two scopes alternated, three rounds, every total kept
        nb = 8
        canv = []
        for i in range(nb):
            pts = torch.from_numpy(synth.lidar_cloud("eight_20cm", seed=300 + i)).to(d)
            vox, coors, npts, num = eng.voxelize(pts)
            canv.append(eng.scatter(eng.pfn(vox, coors, npts, num), coors, num))
        canv = torch.cat(canv)
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

        for rnd in range(3):
            for scope in ("stage3", "rpn"):
                net.train(scope=scope)
                opt = torch.optim.SGD(net.parameters(), lr=1e-3)
                step(opt)
                out.setdefault("step_nb8_" + scope, []).append(step(opt))
        for rnd in range(3):  # the whole "rpn" step per grad-precision mode, alternated
            for m in modes:
                net.train(scope="rpn", grad_precision=m)
                opt = torch.optim.SGD(net.parameters(), lr=1e-3)
                step(opt)
                out.setdefault("step_nb8_rpn_" + m, []).append(step(opt))
        for rnd in range(3):  # the same step with the strided stages and upsamplers in the mode as well, against the units alone
            for m in [m for m in modes if m != "fp32"]:
                for stages in ("units", "rpn"):
                    net.train(scope="rpn", grad_precision=m, grad_stages=stages)
                    opt = torch.optim.SGD(net.parameters(), lr=1e-3)
                    step(opt)
                    out.setdefault(f"step_nb8_rpn_{m}_stages_{stages}", []).append(step(opt))
        # what the forward keeps for the backward, per frame
        net.train(scope="rpn")
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(d)
        y = net.rpn_train(canv)
        torch.cuda.synchronize()
        out["saved_taps_gb_per_frame"] = (torch.cuda.memory_allocated(d) - before) / nb / 1e9
        del y
    print(json.dumps(out))


if __name__ == "__main__":
    main()
