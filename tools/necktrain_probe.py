#!/usr/bin/env python3
"""Kernel time of neck training (csrc/neck_train.hip) on eight_20cm at nb = 1, 8: HIP events around back-to-back C calls whose
arguments are built beforehand, next to each call's floor -- the larger of its algorithmic HBM bytes / 8 TB/s and its executed MFMA
flops / 157.3 TF (the constants bench.py uses).

    python tools/necktrain_probe.py [--frames 1,8] [--reps 10]
    rocprofv3 --kernel-trace --stats -d OUT -o necktrain -- python tools/necktrain_probe.py --frames 8 --no-torch   (per-kernel split:
                                       k_neck_fwd, k_neck_stats, k_neck_dz, k_neck_dw, k_dw_reduce, k_neck_dx, k_gather1)
Also timed in the same run: the same branch in stock PyTorch (conv_transpose2d -> instance_norm -> relu, .backward()), pp_backbone_taps
against pp_backbone, and one whole fine-tuning step at nb = 8 with the neck trained (per-frame forward through pp_backbone_taps, head,
loss, backward of head and neck, SGD step, weight upload).  Prints one JSON line."""
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
CIN, CUP, COFF = (64, 128, 256), (64, 128, 128), (0, 64, 192)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,8")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-torch", action="store_true", help="skip the stock PyTorch yardstick and the whole-step line")
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

    out = {"map": [H, W], "rows": []}
    weights = [net._neck[k].detach().clone() for k in shared.NECK_KEYS]
    for nb in frames:
        y = torch.relu(torch.randn((nb, 320, H, W), device=d, generator=gen))
        dy = torch.randn((nb, 320, H, W), device=d, generator=gen)
        for b in range(3):
            s, h, w = 1 << b, H >> b, W >> b
            p, N, R = h * w, H * W, CUP[b] * s * s
            x = torch.randn((nb, CIN[b], h, w), device=d, generator=gen)
            dw, dx = torch.empty_like(weights[b]), torch.empty_like(x)
            bw = lambda need_dx: lib.pp_neck_backward(ctx, b, ptr(x), ptr(weights[b]), ptr(y), ptr(dy), nb, ptr(dw),  # noqa: E731,B023
                                                      ptr(dx) if need_dx else None, st)  # noqa: B023
            row = {"frames": nb, "branch": b + 1}
            row["neck_backward_ms"] = timed(lambda: bw(True))
            row["neck_backward_dw_only_ms"] = timed(lambda: bw(False))
            # floors.  Bytes: x read by the forward and by dw, y and dy read by the statistics and by dZ, Z written once, read twice and
            # rewritten once as dZ, dZ read by dw and by dx, dx written (the weights and partials are small beside these).
            # Flops: three GEMMs of 2 Cin R p each.
            by = 4.0 * nb * (2 * CIN[b] * p + 4 * CUP[b] * N + 4 * R * p + 2 * R * p + CIN[b] * p)
            fl = 3 * 2.0 * CIN[b] * R * p * nb
            by_nodx = by - 4.0 * nb * (R * p + CIN[b] * p)
            row["floor_ms"] = max(by / HBM_BS, fl / MFMA_FS) * 1e3
            row["floor_bound"] = "bytes" if by / HBM_BS > fl / MFMA_FS else "flops"
            row["floor_dw_only_ms"] = max(by_nodx / HBM_BS, fl * 2 / 3 / MFMA_FS) * 1e3
            if not a.no_torch:
                wt = weights[b].clone().requires_grad_(True)
                xg = x.clone().requires_grad_(True)
                gy = dy[:, COFF[b]:COFF[b] + CUP[b]].contiguous()
                F = torch.nn.functional

                def stock():
                    xg.grad = wt.grad = None  # noqa: B023
                    F.relu(F.instance_norm(F.conv_transpose2d(xg, wt, stride=s), eps=1e-3)).backward(gy)  # noqa: B023
                row["torch_fwd_bwd_ms"] = timed(stock, max(2, a.reps // 2))
            out["rows"].append(row)
            del x, dx
        del y, dy
        torch.cuda.empty_cache()
    out["update_neck_weights_ms"] = timed(lambda: lib.pp_update_neck_weights(ctx, *[ptr(t) for t in weights], st))
    out["update_neck_weights_floor_ms"] = 2 * 4.0 * sum(t.numel() for t in weights) / HBM_BS * 1e3
    gx, gy = int(eng.grid_size[0]), int(eng.grid_size[1])
    canvas = torch.relu(torch.randn((1, 64, gx, gy), device=d, generator=gen)) * (torch.rand((1, 1, gx, gy), device=d, generator=gen) < 0.03)
    rpn = torch.empty((1, 320, H, W), device=d)
    taps = [torch.empty((1, CIN[b], H >> b, W >> b), device=d) for b in range(3)]
    out["backbone_ms"] = timed(lambda: lib.pp_backbone(ctx, ptr(canvas), ptr(rpn), st))
    out["backbone_taps_ms"] = timed(lambda: lib.pp_backbone_taps(ctx, ptr(canvas), ptr(rpn), *[ptr(t) for t in taps], st))
    out["backbone_taps_extra_floor_ms"] = 2 * 4.0 * sum(t.numel() for t in taps) / HBM_BS * 1e3
    if not a.no_torch:
        # one whole fine-tuning step at nb = 8 with the neck trained: canvases of 8 clouds (voxelize, PFN, scatter), then per-frame
        # pp_backbone_taps, head, loss, backward of head and neck, SGD step, weight upload
        nb = 8
        canv = []
        for i in range(nb):
            pts = torch.from_numpy(synth.lidar_cloud("eight_20cm", seed=300 + i)).to(d)
            vox, coors, npts, num = eng.voxelize(pts)
            canv.append(eng.scatter(eng.pfn(vox, coors, npts, num), coors, num))
        canv = torch.cat(canv)
        u = torch.rand((nb, A), device=d, generator=gen)
        ex = {"labels": torch.where(u < 0.002, 1, torch.where(u < 0.3, 0, -1)).to(torch.int32),
              "bbox_targets": torch.randn((nb, A, 7), device=d, generator=gen) * 0.3,
              "dir_targets": (torch.rand((nb, A), device=d, generator=gen) < 0.5).to(torch.int32)}
        lg = lgm.LossGenerator(cfg)
        for scope in ("head", "neck"):
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
