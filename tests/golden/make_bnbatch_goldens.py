#!/usr/bin/env python3
"""Generate tests/golden/bnbatch_small.npz by RUNNING THE REFERENCE with torch autograd on the CPU (needs the reference tree).

    python tests/golden/make_bnbatch_goldens.py

Follows make_bntrain_goldens.py step for step, with the reference's RPN in .train(): the RPN(64) built while torch.nn.InstanceNorm2d is
bound to torch.nn.BatchNorm2d (BatchNorm2d(eps=1e-3, momentum=0.01) in the same positions) and left in train mode, so that every norm
normalises with the statistics of the batch (both frames together) and moves its running statistics.  It runs once in float32 and once
in float64 from the same tensors, canvas and upstream gradient; the float64 values are the goldens, and `ref32_dev_<name>` =
max |v32 - v64| / max |v64| is the reference's own float32 deviation, from which the GPU test takes its bars.

Geometry and draws: make_bntrain_goldens.small_inputs, seed 11 (two frames, canvas [2,64,32,24]); the seed is the first from 11 upward
for which the float32 and the float64 run take the same branch at all nineteen ReLUs (SEED, asserted here and in
tests/test_bnbatch_cpu.py).

Stored, float64: the gradient of every parameter, `g_<i>` in named_parameters() order (57 tensors: the weights at the flattened stride
DW_STRIDE, the norms' weight / bias whole) with `g_<i>_max` and `ref32_dev_g_<i>`; the canvas gradient `dcanvas` at stride DX_STRIDE;
`rpn_out` at stride Y_STRIDE; per norm i in state_dict order the batch statistics `mean_<i>`, `var_<i>` (biased) and the running
statistics after the one forward, `rm_<i>`, `rv_<i>` (`ref32_dev_stats` / `ref32_dev_running`: the largest deviation over the nineteen);
the seed; and `param_names`."""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import REF, ROOT, install_shims, save  # noqa: E402
from make_rpntrain_goldens import DW_STRIDE, DX_STRIDE, dev, split, weight_shapes  # noqa: E402,F401
from make_bntrain_goldens import BN_C, small_inputs  # noqa: E402,F401

SEED = 11
Y_STRIDE = 13


def main():
    install_shims()
    sys.path.insert(0, REF)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    torch.set_num_threads(8)
    import bnbatch_ref as R
    import networks.pointpillars8_shared as net_mod

    def make():
        orig = torch.nn.InstanceNorm2d
        torch.nn.InstanceNorm2d = torch.nn.BatchNorm2d  # make_goldens.py's trick
        try:
            return net_mod.RPN(64).train()
        finally:
            torch.nn.InstanceNorm2d = orig

    probe = make()
    names = [k for k, _ in probe.named_parameters()]
    wnames = [k for k in names if probe.state_dict()[k].dim() == 4]
    bnames = [k[:-len(".running_var")] for k in probe.state_dict() if k.endswith("running_var")]
    assert len(names) == 57 and [tuple(probe.state_dict()[k].shape) for k in wnames] == weight_shapes()
    assert [probe.state_dict()[p + ".weight"].shape[0] for p in bnames] == list(BN_C)
    assert ["rpn." + k for k in names] == list(R.PARAM_KEYS) and ["rpn." + p for p in bnames] == list(R.BN_PREFIXES)
    assert all(m.momentum == R.MOMENTUM and m.eps == R.EPS for m in probe.modules() if isinstance(m, torch.nn.BatchNorm2d))

    def run(dtype, canvas, ws, bn, dy):
        rpn = make().to(dtype)
        sd = {k: torch.from_numpy(w) for k, w in zip(wnames, ws)}
        for p, t in zip(bnames, bn):
            sd.update({p + ".weight": torch.from_numpy(t[0]), p + ".bias": torch.from_numpy(t[1]), p + ".running_mean": torch.from_numpy(t[2]),
                       p + ".running_var": torch.from_numpy(t[3]), p + ".num_batches_tracked": torch.tensor(0)})
        rpn.load_state_dict(sd, strict=True)
        assert rpn.training
        masks, stats = [], {}
        relus = [m for m in rpn.modules() if isinstance(m, torch.nn.ReLU)]
        assert len(relus) == 19
        for m in relus:
            m.register_forward_hook(lambda mod, i, o: masks.append((o.detach() > 0).numpy().copy()))
        for p, m in rpn.named_modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.register_forward_hook(lambda mod, i, o, p=p: stats.__setitem__(p, (i[0].detach().double().mean((0, 2, 3)).numpy(),
                                                                                     i[0].detach().double().var((0, 2, 3), unbiased=False).numpy())))
        x = torch.from_numpy(canvas).to(dtype).requires_grad_(True)
        y = rpn(x)
        y.backward(torch.from_numpy(dy).to(dtype))
        assert len(masks) == 19 and len(stats) == 19
        params = dict(rpn.named_parameters())
        after = rpn.state_dict()
        assert all(int(after[p + ".num_batches_tracked"]) == 1 for p in bnames)
        return dict(masks=masks, g=[params[k].grad.numpy().copy() for k in names], dx=x.grad.numpy().copy(), y=y.detach().numpy().copy(),
                    stats=[stats[p] for p in bnames], run=[(after[p + ".running_mean"].numpy().copy(), after[p + ".running_var"].numpy().copy()) for p in bnames])

    seed = 11
    while True:
        canvas, ws, bn, dy = small_inputs(seed)
        r32, r64 = run(torch.float32, canvas, ws, bn, dy), run(torch.float64, canvas, ws, bn, dy)
        if all(np.array_equal(a, b) for a, b in zip(r32["masks"], r64["masks"])):
            break
        seed += 1
    assert seed == SEED, seed
    # the restatement must agree with the reference's float64 autograd to float64 rounding before anything is written
    wc, wn = split(ws)
    bnd = dict(zip(R.BN_PREFIXES, bn))
    fwd = R.rpn_forward(canvas, wc, wn, bnd)
    rg, rdx = R.rpn_backward(canvas, wc, wn, bnd, fwd, dy)
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()  # noqa: E731
    for k, g in zip(R.PARAM_KEYS, r64["g"]):
        assert rel(rg[k], g) <= 1e-10, (k, rel(rg[k], g))
    assert rel(rdx, r64["dx"]) <= 1e-10 and rel(fwd["y"], r64["y"]) <= 1e-10
    for p, (m, v), (rm, rv), t in zip(R.BN_PREFIXES, r64["stats"], r64["run"], bn):
        sm, sv, n = fwd["stats"][p]
        assert rel(sm, m) <= 1e-10 and rel(sv, v) <= 1e-10, p
        mm, mv = R.moved(t[2], t[3], sm, sv, n)
        assert rel(mm, rm) <= 1e-10 and rel(mv, rv) <= 1e-10, p
    out = dict(seed=seed, param_names=np.array(["rpn." + k for k in names]), dw_stride=DW_STRIDE, dx_stride=DX_STRIDE, y_stride=Y_STRIDE)
    for i, g in enumerate(r64["g"]):
        out[f"g_{i}"] = g.reshape(-1)[::DW_STRIDE].copy() if g.ndim == 4 else g.copy()
        out[f"g_{i}_max"] = float(np.abs(g).max())
        out[f"ref32_dev_g_{i}"] = dev(r32["g"][i], g)
    out["dcanvas"] = r64["dx"].reshape(-1)[::DX_STRIDE].copy()
    out["dcanvas_max"] = float(np.abs(r64["dx"]).max())
    out["ref32_dev_dcanvas"] = dev(r32["dx"], r64["dx"])
    out["rpn_out"] = r64["y"].reshape(-1)[::Y_STRIDE].copy()
    out["rpn_out_max"] = float(np.abs(r64["y"]).max())
    out["ref32_abs_rpn_out"] = float(np.abs(r32["y"].astype(np.float64) - r64["y"]).max())
    sdev, rdev = 0.0, 0.0
    for i in range(19):
        out[f"mean_{i}"], out[f"var_{i}"] = r64["stats"][i]
        out[f"rm_{i}"], out[f"rv_{i}"] = r64["run"][i]
        sdev = max(sdev, *[dev(a, b) for a, b in zip(r32["stats"][i], r64["stats"][i])])
        rdev = max(rdev, *[float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(r32["run"][i], r64["run"][i])])
    out["ref32_dev_stats"], out["ref32_abs_running"] = sdev, rdev
    save("bnbatch_small", **out)
    size = os.path.getsize(os.path.join(HERE, "bnbatch_small.npz"))
    assert size < 700 * 1024, size
    print({k: v for k, v in out.items() if k.startswith("ref32_") or k == "seed"}, size)


if __name__ == "__main__":
    main()
