#!/usr/bin/env python3
"""Whole fine-tuning steps under scope "rpn" at nb = 8 on eight_20cm, per precision of the training forward: train(forward_precision=)
in {fp32, bf16x3, bf16, fp16} x train(grad_precision=) in {fp32, bf16}, each step split into forward (per-frame tapped backbone, head,
loss) and backward + optimizer step + weight upload.  The step is tools/rpntrain_probe.py's: canvases of 8 clouds built beforehand,
SGD, _sync_head / _sync_neck behind the step.  The combinations take turns window by window, so a drift of the clocks reaches all of
them; a window is one untimed step behind the switch of mode (the engine commits the plan of the new mode there, and the first upload
reads the image maps back) and `--steps` steps between HIP events; a figure is the median over `--windows` windows behind one warm-up
round, with the windows' min and max.

The fp32 column calls train() without the new keyword, so `--forward-precision fp32` runs on a tree that has no such keyword: that is
how the column is compared with the commit in front of the feature.

    python tools/autocast_probe.py [--steps 3] [--windows 7] [--forward-precision fp32,bf16x3,bf16,fp16] [--grad-precision fp32,bf16]

Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--forward-precision", default="fp32,bf16x3,bf16,fp16")
    ap.add_argument("--grad-precision", default="fp32,bf16")
    a = ap.parse_args()
    fwds = [m for m in a.forward_precision.split(",") if m]
    grads = [m for m in a.grad_precision.split(",") if m]
    pkg = importlib.import_module("3d_object_detection_amd")
    pkg.install()
    synth = importlib.import_module("3d_object_detection_amd.synth")
    shared = importlib.import_module("3d_object_detection_amd.networks.pointpillars8_shared")
    vgm = importlib.import_module("3d_object_detection_amd.framework.voxel_generator")
    lgm = importlib.import_module("3d_object_detection_amd.framework.loss_generator")
    cfg = synth.load_config("eight_20cm")
    cfg["device"] = torch.device("cuda:0")
    nb = cfg["max_batch"] = 8
    vgm.VoxelGenerator(cfg)
    net = shared.PointPillars(cfg)
    net.load_state_dict(synth.seeded_state_dict(0, cls_bias=-3.0))
    net.profile_stages = False
    eng = net._eng
    d, A = eng.device, eng.A
    gen = torch.Generator(device=d).manual_seed(0)
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

    def steps(opt, n):
        """n steps -> (forward ms, backward + step + upload ms) per step, from events on the stream"""
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(n)]
        for e in ev:
            e[0].record()
            loss = lg.generate(net.heads(net.rpn_train(canv)), ex)["loss"]
            e[1].record()
            opt.zero_grad()
            loss.backward()
            opt.step()
            net._sync_head()
            net._sync_neck()
            e[2].record()
        torch.cuda.synchronize()
        return sum(e[0].elapsed_time(e[1]) for e in ev) / n, sum(e[1].elapsed_time(e[2]) for e in ev) / n

    combos = [(f, g) for f in fwds for g in grads]
    ms = {c: [] for c in combos}
    for win in range(a.windows + 1):  # the first round warms up (tuner, workspaces, clocks) and is dropped
        for f, g in combos:
            if f == "fp32":
                net.float()
                net.train(scope="rpn", grad_precision=g)
            else:
                net.train(scope="rpn", grad_precision=g, forward_precision=f)
            assert eng.effective_precision() == f, (f, eng.effective_precision())
            opt = torch.optim.SGD(net.parameters(), lr=1e-3)
            steps(opt, 1)
            t = steps(opt, a.steps)
            if win:
                ms[f, g].append(t)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    out = {"map": [eng.H, eng.W], "nb": nb, "steps": a.steps, "windows": a.windows, "rows": []}
    for (f, g), v in ms.items():
        fw, bw, tot = [x[0] for x in v], [x[1] for x in v], [x[0] + x[1] for x in v]
        out["rows"].append({"forward_precision": f, "grad_precision": g, "forward_ms": round(med(fw), 3), "backward_step_upload_ms": round(med(bw), 3),
                            "step_ms": round(med(tot), 3), "step_ms_min": round(min(tot), 3), "step_ms_max": round(max(tot), 3),
                            "forward_ms_min": round(min(fw), 3), "forward_ms_max": round(max(fw), 3)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
