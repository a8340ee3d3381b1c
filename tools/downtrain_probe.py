#!/usr/bin/env python3
"""Kernel time of the strided stage backward (csrc/down_train.hip) at block 3's shape on eight_20cm (128 -> 256, 200 x 200 input,
100 x 100 output) at nb = 1, 8, with and without dx: HIP events around back-to-back C calls whose arguments are built beforehand,
next to each call's floors -- its algorithmic HBM bytes / 8 TB/s and its executed MFMA flops / 157.3 TF (the constants bench.py uses).

    python tools/downtrain_probe.py [--frames 1,8] [--reps 10]
    rocprofv3 --kernel-trace --stats -d OUT -o downtrain -- python tools/downtrain_probe.py --frames 8 --no-step   (per-kernel split:
                                       k_conv3_wt, k_down_xpack, k_down_norm, k_conv3_wgrad, k_dw_reduce, k_down_dgrad)
Also timed in the same run: pp_unit_backward at C = 256 on the 100 x 100 map (the yardstick beside it), pp_update_down_weight,
pp_backbone_stage_taps against pp_backbone_block_taps, and whole fine-tuning steps at nb = 8 under scope "block3" and "stage3",
alternated (per-frame forward, head, loss, backward, SGD step, weight upload).  Prints one JSON line."""
import argparse
import ctypes
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BS, MFMA_FS = 8.0e12, 157.3e12
CIN, COUT = 128, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,8")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true", help="skip the whole-step lines")
    a = ap.parse_args()
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
    hin, win, ho, wo = H >> 1, W >> 1, H >> 2, W >> 2
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

    out = {"input": [hin, win], "output": [ho, wo], "cin": CIN, "cout": COUT, "rows": []}
    w0 = net._down[shared.STAGE3_KEY].detach().clone()
    wu = net._block[shared.BLOCK3_KEYS[0]].detach().clone()
    PP = (ho + 2) * (wo + 2)  # positions a product executes per frame: the zero-haloed half-resolution plane
    for nb in frames:
        x = torch.randn((nb, CIN, hin, win), device=d, generator=gen)
        z = torch.randn((nb, COUT, ho, wo), device=d, generator=gen)
        dy = torch.randn((nb, COUT, ho, wo), device=d, generator=gen)
        dw, dx, dwu, du = torch.empty_like(w0), torch.empty_like(x), torch.empty_like(wu), torch.empty_like(z)
        down = lambda need_dx: lib.pp_down_backward(ctx, CIN, COUT, hin, win, ptr(x), ptr(w0), ptr(z), ptr(dy), nb, ptr(dw),  # noqa: E731,B023
                                                    ptr(dx) if need_dx else None, st)  # noqa: B023
        unit = lambda need_du: lib.pp_unit_backward(ctx, COUT, ho, wo, ptr(z), ptr(wu), ptr(dy), ptr(dy), nb, ptr(dwu),  # noqa: E731,B023
                                                    ptr(du) if need_du else None, st)  # noqa: B023
        row = {"frames": nb}
        for rep in range(2):  # the two entry points alternated, twice: the second round is the one reported
            row["down_backward_ms"] = timed(lambda: down(True))
            row["unit_backward_ms"] = timed(lambda: unit(True))
            row["down_backward_dw_only_ms"] = timed(lambda: down(False))
            row["unit_backward_dw_only_ms"] = timed(lambda: unit(False))
        # floors.  Tensor passes: x read and its four parity planes (together one x) written, z and dy read and dz written, the planes
        # and dz read by the wgrad (3 nx + 4 nz); with dx, dz read again and dx written (4 nx + 5 nz); padded planes counted as tight
        # ones, the weights and partials are small beside these.  Executed flops: 2 Cout 9 Cin PP per product and frame.
        nx, nz = float(nb) * CIN * hin * win, float(nb) * COUT * ho * wo
        fl = 2.0 * COUT * 9 * CIN * PP * nb
        row["floor_flops_ms"], row["floor_bytes_ms"] = 2 * fl / MFMA_FS * 1e3, 4.0 * (4 * nx + 5 * nz) / HBM_BS * 1e3
        row["floor_flops_dw_only_ms"], row["floor_bytes_dw_only_ms"] = fl / MFMA_FS * 1e3, 4.0 * (3 * nx + 4 * nz) / HBM_BS * 1e3
        out["rows"].append(row)
        del x, z, dy, dx, du
        torch.cuda.empty_cache()
    out["update_down_weight_ms"] = timed(lambda: lib.pp_update_down_weight(ctx, 2, ptr(w0), st))
    out["update_down_weight_floor_ms"] = 4.0 * w0.numel() * 3 / HBM_BS * 1e3  # the weight read, its image written, the map read
    out["down_tiling"] = [t["tiling"] for t in eng.layer_tilings() if t["kind"] == 0 and t["level"] == 2 and t["stride"] == 2]
    gx, gy = int(eng.grid_size[0]), int(eng.grid_size[1])
    canvas = torch.relu(torch.randn((1, 64, gx, gy), device=d, generator=gen)) * (torch.rand((1, 1, gx, gy), device=d, generator=gen) < 0.03)
    rpn = torch.empty((1, 320, H, W), device=d)
    taps = [torch.empty((1, 64 << b, H >> b, W >> b), device=d) for b in range(3)]
    units, z3 = torch.empty((5, COUT, ho, wo), device=d), torch.empty((1, COUT, ho, wo), device=d)
    for rep in range(2):
        out["backbone_block_taps_ms"] = timed(lambda: lib.pp_backbone_block_taps(ctx, ptr(canvas), ptr(rpn), *[ptr(t) for t in taps], ptr(units), st))
        out["backbone_stage_taps_ms"] = timed(lambda: lib.pp_backbone_stage_taps(ctx, ptr(canvas), ptr(rpn), *[ptr(t) for t in taps], ptr(units),
                                                                                 ptr(z3), st))
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
            for scope in ("block3", "stage3"):
                net.train(scope=scope)
                opt = torch.optim.SGD(net.parameters(), lr=1e-3)
                step(opt)
                out.setdefault("step_nb8_" + scope, []).append(step(opt))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
