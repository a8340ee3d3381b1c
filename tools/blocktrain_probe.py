#!/usr/bin/env python3
"""Kernel time of block-3 training (csrc/block_train.hip) on eight_20cm (C = 256 on the 100 x 100 map) at nb = 1, 8: HIP events around
back-to-back C calls whose arguments are built beforehand, next to each call's floor -- the larger of its algorithmic HBM bytes / 8 TB/s
and its executed MFMA flops / 157.3 TF (the constants bench.py uses).

    python tools/blocktrain_probe.py [--frames 1,8] [--reps 10]
    rocprofv3 --kernel-trace --stats -d OUT -o blocktrain -- python tools/blocktrain_probe.py --frames 8 --no-torch   (per-kernel split:
                                       k_conv3_wt, k_unit_pack, k_conv3_wgrad, k_dw_reduce, k_unit_dgrad, k_unit_norm, k_unit_image)
Also timed in the same run: the same unit in stock PyTorch (instance_norm -> relu -> conv2d, .backward()), pp_update_block_weights,
pp_backbone_block_taps against pp_backbone_taps, and one whole fine-tuning step at nb = 8 per scope (per-frame forward, head, loss,
backward, SGD step, weight upload).  Prints one JSON line."""
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
C = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,8")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-torch", action="store_true", help="skip the stock PyTorch yardstick and the whole-step lines")
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
    h, w = H >> 2, W >> 2
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

    out = {"map": [h, w], "C": C, "rows": []}
    weights = [net._block[k].detach().clone() for k in shared.BLOCK3_KEYS]
    wt = weights[0]
    for nb in frames:
        u = torch.randn((nb, C, h, w), device=d, generator=gen)
        dy = torch.randn((nb, C, h, w), device=d, generator=gen)
        dw, du = torch.empty_like(wt), torch.empty_like(u)
        bw = lambda need_du: lib.pp_unit_backward(ctx, C, h, w, ptr(u), ptr(wt), ptr(dy), ptr(dy), nb, ptr(dw),  # noqa: E731,B023
                                                  ptr(du) if need_du else None, st)  # noqa: B023
        row = {"frames": nb}
        row["unit_backward_ms"] = timed(lambda: bw(True))
        row["unit_backward_dw_only_ms"] = timed(lambda: bw(False))
        # floors.  Bytes per plane element: u and dy read and a, dz written by the pack; a and dz read by the wgrad; dz read and da
        # written by the dgrad; da, a, u, dskip read and du written by the norm backward (two passes over da and a) -- 6 / 17 tensor
        # passes without / with du, padded planes counted as tight ones; the weights and partials are small beside these.
        # Flops: two products of 2 C C 9 h w each.
        n = float(nb) * C * h * w
        fl = 2.0 * C * C * 9 * h * w * nb
        row["floor_ms"] = max(4.0 * 17 * n / HBM_BS, 2 * fl / MFMA_FS) * 1e3
        row["floor_dw_only_ms"] = max(4.0 * 6 * n / HBM_BS, fl / MFMA_FS) * 1e3
        row["floor_bound"] = "bytes" if 4.0 * 17 * n / HBM_BS > 2 * fl / MFMA_FS else "flops"
        if not a.no_torch:
            wg = wt.clone().requires_grad_(True)
            ug = u.clone().requires_grad_(True)
            F = torch.nn.functional

            def stock():
                ug.grad = wg.grad = None  # noqa: B023
                (ug + F.conv2d(F.relu(F.instance_norm(ug, eps=1e-3)), wg, padding=1)).backward(dy)  # noqa: B023
            row["torch_fwd_bwd_ms"] = timed(stock, max(2, a.reps // 2))

            def stock_fwd():
                with torch.no_grad():
                    u + F.conv2d(F.relu(F.instance_norm(u, eps=1e-3)), wt, padding=1)  # noqa: B023
            row["torch_fwd_ms"] = timed(stock_fwd, max(2, a.reps // 2))
        out["rows"].append(row)
        del u, dy, du
        torch.cuda.empty_cache()
    arr = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in weights])
    out["update_block_weights_ms"] = timed(lambda: lib.pp_update_block_weights(ctx, 2, arr, 5, st))
    out["update_block_weights_floor_ms"] = 4.0 * sum(t.numel() for t in weights) * (1 + 36 / 9 * 2) / HBM_BS * 1e3  # g read; U and its map at 36 / 9 of g
    out["block3_tilings"] = [t["tiling"] for t in eng.layer_tilings() if t["kind"] == 0 and t["level"] == 2 and t["stride"] == 1]
    gx, gy = int(eng.grid_size[0]), int(eng.grid_size[1])
    canvas = torch.relu(torch.randn((1, 64, gx, gy), device=d, generator=gen)) * (torch.rand((1, 1, gx, gy), device=d, generator=gen) < 0.03)
    rpn = torch.empty((1, 320, H, W), device=d)
    taps = [torch.empty((1, 64 << b, H >> b, W >> b), device=d) for b in range(3)]
    units = torch.empty((5, C, h, w), device=d)
    out["backbone_taps_ms"] = timed(lambda: lib.pp_backbone_taps(ctx, ptr(canvas), ptr(rpn), *[ptr(t) for t in taps], st))
    out["backbone_block_taps_ms"] = timed(lambda: lib.pp_backbone_block_taps(ctx, ptr(canvas), ptr(rpn), *[ptr(t) for t in taps], ptr(units), st))
    out["backbone_block_taps_extra_floor_ms"] = 2 * 4.0 * units.numel() / HBM_BS * 1e3
    if not a.no_torch:
        # one whole fine-tuning step at nb = 8 per scope: canvases of 8 clouds (voxelize, PFN, scatter), then per-frame backbone, head,
        # loss, backward, SGD step, weight upload
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
        for scope in ("head", "neck", "block3"):
            net.train(scope=scope)
            opt = torch.optim.SGD(net.parameters(), lr=1e-3)
            parts = {}

            def step():
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                ev[0].record()
                rpn = net.rpn_train(canv)
                ev[1].record()
                loss = lg.generate(net.heads(rpn), ex)["loss"]  # noqa: B023
                ev[2].record()
                opt.zero_grad()  # noqa: B023
                loss.backward()
                opt.step()  # noqa: B023
                net._sync_head()
                net._sync_neck()
                ev[3].record()
                torch.cuda.synchronize()
                for k, i in (("backbone_forward_ms", 0), ("head_and_loss_ms", 1), ("backward_step_upload_ms", 2)):
                    parts[k] = ev[i].elapsed_time(ev[i + 1])  # noqa: B023
            step()
            step()
            out["step_nb8_" + scope] = dict(parts, total_ms=sum(parts.values()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
