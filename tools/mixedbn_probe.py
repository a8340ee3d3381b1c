#!/usr/bin/env python3
"""Kernel time of the mixed-precision BatchNorm backwards on eight_20cm: pp_{unit,down,neck}_backward_{affine,bn}_mp at the three level
shapes (unit (64, 400 x 400), (128, 200 x 200), (256, 100 x 100); stage (64 -> 64, 800 x 800 in), (64 -> 128, 400 x 400 in), (128 -> 256,
200 x 200 in); the three branches of the map), with du / dx and the two sums, at nb = 1 and 8, in modes 0 (fp32: the fp32 sibling of the
same build, in the same process), 1 (bf16x3) and 2 (bf16).  The method is tools/rpntrain_probe.py's: HIP events around back-to-back C
calls whose arguments are built beforehand; a figure is the median of `--windows` event windows of `--reps` calls each, taken after a
warm-up round; the levels, forms and modes take turns window by window, so a drift of the clocks reaches all of them, and every row
carries its windows' min and max.  `vs_fp32` is median / mode 0's median and `ships` whether the mode's slowest window beats mode 0's
fastest (the rule by which pp_unit_backward_bn_path hands a shape to a mode).

Then whole fine-tuning steps of networks.pointpillars8_export at nb = 8 under scope "rpn", grad_stages="rpn", bn_stats "frozen" and
"moving", per bn_grad_precision mode, alternated, three rounds (forward, head, loss, backward, SGD step, weight upload and fold).

Every step that uses the GPU (the calls at one nb, the whole steps) runs in a child process of its own under its own time limit; after
a step that fails or runs out of time nothing more is started.  Prints one JSON line.

    python tools/mixedbn_probe.py [--frames 1,8] [--reps 10] [--windows 5] [--no-step] [--limit 420]"""
import argparse
import ctypes
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODES = {"fp32": 0, "bf16x3": 1, "bf16": 2}
FORMS = ("affine", "bn")


def setup(max_batch):
    import torch
    importlib.import_module("3d_object_detection_amd").install()
    synth = importlib.import_module("3d_object_detection_amd.synth")
    vgm = importlib.import_module("3d_object_detection_amd.framework.voxel_generator")
    cfg = synth.load_config("eight_20cm")
    cfg["device"] = torch.device("cuda:0")
    cfg["max_batch"] = max_batch
    vgm.VoxelGenerator(cfg)
    net = importlib.import_module("3d_object_detection_amd.networks.pointpillars8_export").PointPillars(cfg)
    net.load_state_dict(synth.seeded_state_dict(0, norm="batch", cls_bias=-3.0))
    return torch, synth, cfg, net


def timed(torch, fn, reps):
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


def step_calls(a, nb):
    torch, _, _, net = setup(max(nb, 1))
    eng = net._eng
    d, H, W = eng.device, eng.H, eng.W
    lib, ctx, st = eng.lib, eng.ctx, torch.cuda.current_stream().cuda_stream
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    gen = torch.Generator(device=d).manual_seed(0)
    rnd = lambda *s: torch.randn(s, device=d, generator=gen)  # noqa: E731
    yn, dyn = rnd(nb, 320, H, W), rnd(nb, 320, H, W)
    calls, keep = {}, [yn, dyn]
    for b in (2, 1, 0):
        C, cin, h, w = 64 << b, eng.DOWN_PAIRS[b][0], H >> b, W >> b
        cup = 128 if b else 64
        wu, w0, wn = (rnd(C, C, 3, 3) * 0.05).contiguous(), (rnd(C, cin, 3, 3) * 0.05).contiguous(), (rnd(C, cup, 1 << b, 1 << b) * 0.05).contiguous()
        x, z, dy = rnd(nb, cin, 2 * h, 2 * w), rnd(nb, C, h, w), rnd(nb, C, h, w)
        # per-channel norms: scale around 1, shift, and statistics that go with unit-variance inputs
        norm = {n: [torch.rand(n, device=d, generator=gen) + 0.5, rnd(n) * 0.1, rnd(n) * 0.1, torch.rand(n, device=d, generator=gen) + 0.5] for n in {C, cup}}
        dwu, dw0, dwn, du, dx = torch.empty_like(wu), torch.empty_like(w0), torch.empty_like(wn), torch.empty_like(z), torch.empty_like(x)
        dxn = torch.empty_like(z)
        sums = [torch.empty(256, device=d, dtype=torch.float64) for _ in range(2)]
        keep += [wu, w0, wn, x, z, dy, norm, dwu, dw0, dwn, du, dx, dxn, sums]
        for form in FORMS:
            nt = lambda n, form=form, norm=norm: [ptr(t) for t in norm[n][:2 if form == "affine" else 4]]  # noqa: E731
            tail = [] if form == "affine" else [0]
            for m, mode in MODES.items():
                assert getattr(lib, "pp_unit_backward_bn_path")(ctx, mode, C, h, w) in (mode, 0)
                calls[("unit", form, m, b)] = lambda C=C, h=h, w=w, z=z, wu=wu, dy=dy, dwu=dwu, du=du, nt=nt, tail=tail, mode=mode, form=form: getattr(
                    lib, f"pp_unit_backward_{form}_mp")(ctx, mode, C, h, w, ptr(z), ptr(wu), *nt(C), ptr(dy), ptr(dy), nb, ptr(dwu), ptr(du),
                                                        ptr(sums[0]), ptr(sums[1]), *tail, st)
                calls[("down", form, m, b)] = lambda C=C, cin=cin, h=h, w=w, x=x, w0=w0, z=z, dy=dy, dw0=dw0, dx=dx, nt=nt, tail=tail, mode=mode, \
                    form=form: getattr(
                    lib, f"pp_down_backward_{form}_mp")(ctx, mode, cin, C, 2 * h, 2 * w, ptr(x), ptr(w0), ptr(z), *nt(C), ptr(dy), nb, ptr(dw0), ptr(dx),
                                                        ptr(sums[0]), ptr(sums[1]), *tail, st)
                calls[("neck", form, m, b)] = lambda b=b, cup=cup, z=z, wn=wn, dwn=dwn, dxn=dxn, nt=nt, tail=tail, mode=mode, form=form: getattr(
                    lib, f"pp_neck_backward_{form}_mp")(ctx, mode, b, ptr(z), ptr(wn), *nt(cup), ptr(yn), ptr(dyn), nb, ptr(dwn), ptr(dxn),
                                                        ptr(sums[0]), ptr(sums[1]), *tail, st)
    ms = {k: [] for k in calls}
    for win in range(a.windows + 1):  # the first round warms up (workspaces grow, clocks rise) and is dropped
        for k, fn in calls.items():
            t = timed(torch, fn, a.reps)
            if win:
                ms[k].append(t)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    rows = []
    for (fam, form, m, b), v in ms.items():
        f32 = ms[(fam, form, "fp32", b)]
        C, h, w = 64 << b, H >> b, W >> b
        path = lib.pp_unit_backward_bn_path(ctx, MODES[m], C, h, w) if fam == "unit" else MODES[m]
        rows.append(dict(frames=nb, call=f"{fam}_backward_{form}_mp", level=b, grad_precision=m, path=path, ms=med(v), ms_min=min(v), ms_max=max(v),
                         **({} if m == "fp32" else dict(vs_fp32=med(v) / med(f32), ships=max(v) < min(f32)))))
    return dict(rows=rows)


def step_train(a):
    torch, synth, cfg, net = setup(8)
    lgm = importlib.import_module("3d_object_detection_amd.framework.loss_generator")
    eng = net._eng
    d, A, nb = eng.device, eng.A, 8
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

    out = {}
    for rnd in range(3):
        for stats in ("frozen", "moving"):
            for m in MODES:
                net.train(scope="rpn", bn_stats=stats, bn_grad_precision=m, grad_stages="rpn")
                opt = torch.optim.SGD(net.parameters(), lr=1e-3)
                step(opt)
                out.setdefault(f"step_nb8_rpn_{stats}_{m}", []).append(step(opt))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,8")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="skip the whole-step lines")
    ap.add_argument("--limit", type=int, default=420, help="seconds a step may take")
    ap.add_argument("--step", default=None, help="(internal) run one step in this process: calls:<nb> or train")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step_train(a) if a.step == "train" else step_calls(a, int(a.step.split(":")[1]))))
        return 0
    out = {"reps": a.reps, "windows": a.windows, "rows": []}
    steps = [f"calls:{int(v)}" for v in a.frames.split(",") if v] + ([] if a.no_step else ["train"])
    for s in steps:  # a fresh child per step under its own time limit; a failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--step", s, "--reps", str(a.reps), "--windows", str(a.windows)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            out["failed"] = dict(step=s, why=f"no result within {a.limit} s")
            break
        if r.returncode != 0:
            out["failed"] = dict(step=s, rc=r.returncode, stderr=r.stderr[-2000:])
            break
        got = json.loads(r.stdout.strip().splitlines()[-1])
        out["rows"] += got.pop("rows", [])
        out.update(got)
    print(json.dumps(out))
    return 1 if "failed" in out else 0


if __name__ == "__main__":
    sys.exit(main())
