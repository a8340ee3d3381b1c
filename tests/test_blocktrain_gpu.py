"""GPU: the Resnet unit backward, block 3's unit taps and the in-place update of block 3's packed weights (csrc/block_train.hip,
pp_backbone_block_taps in csrc/conv_run.hip) through the engine wrappers of the C ABI and through the autograd surface
(PointPillars.train(scope="block3")), against the reference's float64 autograd goldens (tests/golden/make_blocktrain_goldens.py) and
the float64 restatement pinned to them (tests/blocktrain_ref.py).

Bars.  Fixture gradients: 4 x ref32_dev x max |g64| per tensor, ref32_dev being the reference's own float32-against-float64 deviation
stored in the fixture (the project's bar for gradients, test_headtrain_gpu.check_grad).  Everything else: the element-wise a-priori
bound of blocktrain_ref.grad_bounds (float32 summation in any order plus the float32 evaluation of a and du from float32 inputs).
Equality is asserted between identical calls, with and without du, for a frame's du whatever batch it rides in, for the dskip add,
between the autograd surface and the same calls made by hand, and between an engine whose block-3 images were rewritten in place and
a fresh engine that committed the same values.  Random inputs go through blocktrain_ref.tie_free, so no ReLU argument lies within
1e-4 of zero (asserted)."""
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden, load_pkg
import blocktrain_ref as R
from train_common import (GX, GY, canvases_of, check_bound, check_grad, dev, engine, loaded, random_case, small_cfg, small_net,  # noqa: F401
                          two_frames)

sys.path.insert(0, GOLDEN)
from make_blocktrain_goldens import DW_STRIDE, MODULES, small_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = load_pkg("engine").Engine.BLOCK3_KEYS  # unit order a .. e


# ------------------------------------------------------------------ 1. fixture gradients
@pytest.mark.parametrize("name", list(MODULES))
def test_fixture_gradients(name):
    g = golden("blocktrain_small")
    x, ws, dy = small_inputs(name)
    eng = engine()
    us = [g[f"u_{name}_{k}"] for k in range(len(ws))]
    assert np.array_equal(us[0], x)
    dyd = dev(dy)
    if len(ws) == 1:  # x + U(x)
        dw, dx = eng.unit_backward(dev(us[0]), dev(ws[0]), dyd, dskip=dyd)
        dws = [dw]
        rdw, rdx = R.unit_backward(us[0], ws[0], dy, dskip=dy)
        rdws = [rdw]
    else:             # x + U_b(U_a(x)), chained by hand: unit a is fed the GPU's own gradient of m = U_a(x)
        dwb, gm = eng.unit_backward(dev(us[1]), dev(ws[1]), dyd)
        dwa, dx = eng.unit_backward(dev(us[0]), dev(ws[0]), gm, dskip=dyd)
        dws = [dwa, dwb]
        rdwb, rgm = R.unit_backward(us[1], ws[1], dy)
        rdwa, rdx = R.unit_backward(us[0], ws[0], rgm, dskip=dy)
        rdws = [rdwa, rdwb]
    dx_max = np.abs(g["dx_" + name]).max()
    check_grad(dx, g["dx_" + name], float(g["ref32_dev_dx_" + name]), dx_max, f"golden dx {name}")
    check_grad(dx, rdx, float(g["ref32_dev_dx_" + name]), dx_max, f"restated dx {name}")  # every element
    for k, dw in enumerate(dws):
        dw_max, d = float(g[f"dw_{name}_{k}_max"]), float(g[f"ref32_dev_dw_{name}_{k}"])
        check_grad(dw.reshape(-1)[::DW_STRIDE[name]], g[f"dw_{name}_{k}"], d, dw_max, f"golden dw {name} unit {k}")
        check_grad(dw, rdws[k], d, dw_max, f"restated dw {name} unit {k}")


# ------------------------------------------------------------------ 2. shapes: tile edges, halos, K ranges
@pytest.mark.parametrize("C,h,w,nb", [(64, 33, 17, 1), (128, 20, 18, 2), (256, 25, 9, 3), (256, 1, 7, 2), (256, 2, 20, 1), (256, 3, 2, 2)])
def test_shapes(C, h, w, nb):
    eng = engine()
    u, wt, dz, dskip = random_case(C, h, w, nb, 100 + C + h)
    ud, wd, dzd, dsd = dev(u), dev(wt), dev(dz), dev(dskip)
    dw, du = eng.unit_backward(ud, wd, dzd)
    rw, ru, bw, bu, ties = R.grad_bounds(u, wt, dz)
    assert not ties.any()
    check_bound(dw, rw, bw, f"{C}x{h}x{w}x{nb} dw")
    check_bound(du, ru, bu, f"{C}x{h}x{w}x{nb} du")
    dw2, du2 = eng.unit_backward(ud, wd, dzd)
    dw3, none = eng.unit_backward(ud, wd, dzd, need_du=False)
    assert none is None and torch.equal(dw, dw2) and torch.equal(du, du2) and torch.equal(dw, dw3)
    dw4, du4 = eng.unit_backward(ud, wd, dzd, dskip=dsd)
    assert torch.equal(dw, dw4) and torch.equal(du4, du + dsd)  # dskip is exactly one fp32 add
    rw, ru, bw, bu, _ = R.grad_bounds(u, wt, dz, dskip=dskip)
    check_bound(du4, ru, bu, f"{C}x{h}x{w}x{nb} du + dskip")


# ------------------------------------------------------------------ 3. frames
def test_frames():
    C, h, w, nb = 128, 12, 10, 2
    eng = engine()
    u, wt, dz, dskip = random_case(C, h, w, nb, 7)
    dw, du = eng.unit_backward(dev(u), dev(wt), dev(dz), dskip=dev(dskip))
    total = np.zeros(wt.shape)
    bound = R.grad_bounds(u, wt, dz)[2]
    for f in range(nb):
        s = slice(f, f + 1)
        dwf, duf = eng.unit_backward(dev(u[s]), dev(wt), dev(dz[s]), dskip=dev(dskip[s]))
        assert torch.equal(duf[0], du[f]), f  # a frame's du does not depend on the batch it rides in
        total += dwf.cpu().numpy().astype(np.float64)
        bound = bound + R.grad_bounds(u[s], wt, dz[s])[2]
    check_bound(dw, total, bound, "frames dw")


# ------------------------------------------------------------------ 4. unit taps of block 3
def test_backbone_block_taps(loaded):  # noqa: F811
    eng, sd, canvas = loaded["eng"], loaded["sd"], loaded["canvas"]
    want = eng.backbone_taps(canvas)
    got = eng.backbone_block_taps(canvas)
    assert len(got) == 5 and all(torch.equal(a, b) for a, b in zip(got[:4], want))
    assert torch.equal(eng.backbone(canvas), got[0])
    units = got[4].cpu().numpy().astype(np.float64)
    assert units.shape == (5, 256, 6, 4)
    ws = [sd[k].astype(np.float64) for k in KEYS]
    h = units[0:1]
    m3 = R.unit_forward(h, ws[0])
    r3 = h + R.unit_forward(m3, ws[1])
    m4 = R.unit_forward(r3, ws[2])
    r4 = r3 + R.unit_forward(m4, ws[3])
    x3 = r4 + R.unit_forward(r4, ws[4])
    for name, a, b in (("m3", m3, units[1:2]), ("r3", r3, units[2:3]), ("m4", m4, units[3:4]), ("r4", r4, units[4:5]),
                       ("x3", x3, got[3].cpu().numpy())):
        err = np.abs(a - b).max()
        print(f"{name}: restated forward against the tap {err:.3e} (max |tap| {np.abs(b).max():.3f})")
        assert err <= 2e-4, name  # the project's backbone bar
    assert np.abs(units[0]).max() > 0 and units[0].min() >= 0  # h is behind a ReLU


# ------------------------------------------------------------------ 5. weight update
UX, UY = 64, 32  # cells: the level-2 map is 8 x 4, whole 4 x 4 tiles, so that wino6 can be forced too


@pytest.mark.parametrize("force", [None, "wino6 tw4", "wino4 tw4 bx2", "wino tw8", "k3s1 tw8 w2x2 t4x5"])
def test_update_block_weights(force, monkeypatch):
    if force:
        monkeypatch.setenv("PP_FORCE_VARIANT", force)  # ahead of the engines: the tuner reads it at commit time
    load_pkg().install()
    synth = load_pkg("synth")
    sd = {k: np.asarray(v, np.float32) for k, v in synth.seeded_state_dict(0).items()}
    eng = load_pkg("engine").Engine(small_cfg(UX, UY, 2))
    eng.load_state_dict(sd)
    til = eng.layer_tilings()
    block3 = [t for t in til if t["kind"] == 0 and t["level"] == 2 and t["stride"] == 1]
    print(force, [t["tiling"] for t in block3])
    assert len(block3) == 5 and all(force is None or force in t["tiling"] for t in block3)  # the forced tiling is the one that runs
    rng = np.random.default_rng(5)
    canvas = np.zeros((1, 64, UX, UY), np.float32)
    cells = rng.choice(UX * UY, 300, replace=False)
    canvas[0, :, cells // UY, cells % UY] = np.maximum(rng.standard_normal((300, 64)), 0).astype(np.float32)
    canvas = dev(canvas)
    pts = dev(rng.uniform([0, 0, -1.5, 0], [0.2 * UX, 0.2 * UY, 1.0, 1], (6000, 4)).astype(np.float32))
    base = eng.backbone(canvas)
    new = dict(sd)
    for k in KEYS:
        new[k] = sd[k] + rng.standard_normal(sd[k].shape).astype(np.float32) * np.float32(0.02)
    eng.update_block_weights({k: dev(sd[k]) for k in KEYS})  # the committed values again: the images must not change
    assert torch.equal(eng.backbone(canvas), base)
    eng.infer_frame(pts)
    old_rpn = eng.fetch(0, "rpn").clone()
    eng.update_block_weights({k: dev(new[k]) for k in KEYS})
    got = eng.backbone(canvas)
    eng.infer_frame(pts)
    got_rpn = eng.fetch(0, "rpn").clone()
    fresh = load_pkg("engine").Engine(small_cfg(UX, UY, 2))  # same shapes: same tilings, same packing, same kernels
    fresh.load_state_dict(new)
    assert fresh.layer_tilings() == til
    assert torch.equal(fresh.backbone(canvas), got)
    fresh.infer_frame(pts)
    assert torch.equal(fresh.fetch(0, "rpn"), got_rpn)
    assert (got - base).abs().max() > 1e-3 and (got_rpn - old_rpn).abs().max() > 1e-3
    eng.update_block_weights({k: dev(sd[k]) for k in KEYS})
    assert torch.equal(eng.backbone(canvas), base)


# ------------------------------------------------------------------ 6 / 7. autograd surface and trajectory
def test_autograd_surface():
    load_pkg().install()
    net, _ = small_net()
    eng = net._eng
    shared = load_pkg("networks.pointpillars8_shared")
    assert shared.BLOCK3_KEYS is eng.BLOCK3_KEYS and len(KEYS) == 5
    example = two_frames(eng)
    plain = net(example)
    assert all(v.grad_fn is None for v in plain.values())
    net.train(scope="block3")
    names = [k for k, _ in net.named_parameters()]
    assert names == list(shared.BLOCK3_KEYS + shared.NECK_KEYS + shared.HEAD_KEYS)
    assert all(p.is_cuda and p.requires_grad for p in net.parameters())
    preds = net(example)
    for k in plain:
        assert preds[k].requires_grad and torch.equal(preds[k].detach(), plain[k]), k
    rng = np.random.default_rng(8)
    up = {k: dev(rng.standard_normal(tuple(v.shape)).astype(np.float32) * np.float32(1e-2)) for k, v in preds.items()}
    net.zero_grad()
    sum((preds[k] * up[k]).sum() for k in preds).backward()
    # the same by hand
    taps = [eng.backbone_block_taps(c) for c in canvases_of(eng, example)]
    y, x1, x2, x3 = (torch.cat([t[i] for t in taps]) for i in range(4))
    units = [torch.stack([t[4][k] for t in taps]) for k in range(5)]
    assert torch.equal(y, net.rpn_train(torch.cat(canvases_of(eng, example))).detach())
    assert torch.equal(y, torch.cat([net.rpn(c) for c in canvases_of(eng, example)]))
    gh, dxh = eng.head_backward(y, up["cls_preds"], up["box_preds"], up["dir_preds"])
    params = dict(net.named_parameters())
    for k in shared.HEAD_KEYS:
        assert torch.equal(params[k].grad, gh[k].reshape(params[k].shape)), k
    g = None
    for b, x in enumerate((x1, x2, x3)):
        p = params[shared.NECK_KEYS[b]]
        dw, dx = eng.neck_backward(b, x, p.detach(), y, dxh, need_dx=(b == 2))
        assert p.grad is not None and torch.equal(p.grad, dw), b
        g = dx
    wb = [params[k].detach() for k in shared.BLOCK3_KEYS]
    h, m3, r3, m4, r4 = units
    dws = [None] * 5
    dws[4], g_r4 = eng.unit_backward(r4, wb[4], g, dskip=g)
    dws[3], g_m4 = eng.unit_backward(m4, wb[3], g_r4)
    dws[2], g_r3 = eng.unit_backward(r3, wb[2], g_m4, dskip=g_r4)
    dws[1], g_m3 = eng.unit_backward(m3, wb[1], g_r3)
    dws[0], none = eng.unit_backward(h, wb[0], g_m3, need_du=False)
    assert none is None
    dys = [g_m3, g_r3, g_m4, g_r4, g]
    for k, key in enumerate(shared.BLOCK3_KEYS):
        assert params[key].grad is not None and torch.equal(params[key].grad, dws[k]), key
        rw, _, bw, _, ties = R.grad_bounds(units[k].cpu().numpy(), wb[k].cpu().numpy(), dys[k].cpu().numpy())
        print(f"unit {k}: {int(ties.sum())} near-ties of {ties.size}")
        assert ties.sum() <= 1e-3 * ties.size, key
        check_bound(params[key].grad, rw, bw, f"autograd dw unit {k}")
    net.train()
    assert [k for k, _ in net.named_parameters()] == list(shared.HEAD_KEYS)
    assert not any(p.requires_grad for p in list(net._neck.values()) + list(net._block.values()))


def test_trajectory():
    """Twenty Adam steps (lr 1e-3, clip_grad_norm_ 10: the reference loop's calls) on a fixed batch of two frames: training block 3
    with the neck and the head lowers the loss, state_dict() returns the stepped block, and a fresh network loaded with it computes
    the same backbone output.  The final losses of "block3" and "neck" are printed side by side; which is lower is not asserted."""
    load_pkg().install()
    LossGenerator = load_pkg("framework.loss_generator").LossGenerator
    final = {}
    for scope in ("block3", "neck"):
        net, cfg = small_net()
        eng = net._eng
        example = two_frames(eng)
        rng = np.random.default_rng(21)
        u = rng.random((2, eng.A))
        labels = np.where(u < 1 / 7, 1, np.where(u < 0.75, 0, -1)).astype(np.int32)
        ex = {"labels": labels, "bbox_targets": (rng.standard_normal((2, eng.A, 7)) * 0.4).astype(np.float32) * (labels > 0)[..., None],
              "dir_targets": (rng.random((2, eng.A)) < 0.5).astype(np.int32)}
        lg = LossGenerator(cfg)
        net.train(scope=scope)
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        losses = []
        for _ in range(20):
            loss = lg.generate(net(example), ex)["loss"]
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(list(net.parameters()), 10.0)
            opt.step()
            losses.append(float(loss))
        with torch.no_grad():
            losses.append(float(lg.generate(net(example), ex)["loss"]))
        print(scope, " ".join(f"{v:.6f}" for v in losses))
        assert np.isfinite(losses).all() and losses[-1] < losses[0], (scope, losses)
        final[scope] = losses
        if scope == "block3":
            sd = net.state_dict()
            start = load_pkg("synth").seeded_state_dict(0)
            for k in KEYS:  # state_dict returns the stepped block
                assert np.abs(sd[k] - np.asarray(start[k], np.float32).reshape(sd[k].shape)).max() > 1e-4, k
            canvas = canvases_of(eng, example)[0]
            want = net.rpn(canvas)
            other, _ = small_net()
            other.load_state_dict(sd)
            assert torch.equal(other.rpn(canvas), want)
    assert final["block3"][0] == final["neck"][0]
    print("final loss: block3", final["block3"][-1], "neck", final["neck"][-1])


# ------------------------------------------------------------------ 8. errors
def test_bad_arguments_raise_and_the_next_call_works(loaded):  # noqa: F811
    eng = engine(2)
    u, wt, dz, dskip = random_case(64, 5, 4, 2, 1)
    args = [dev(u), dev(wt), dev(dz)]
    good = eng.unit_backward(*args, dskip=dev(dskip))
    with pytest.raises(TypeError):
        eng.unit_backward(args[0].double(), *args[1:])
    with pytest.raises(TypeError):
        eng.unit_backward(args[0], args[1].cpu(), args[2])
    with pytest.raises(TypeError):
        eng.unit_backward(*args, dskip=dskip)
    with pytest.raises(ValueError):
        eng.unit_backward(args[0], args[1], args[2][:, :, :, :-1])
    with pytest.raises(ValueError):
        eng.unit_backward(args[0], args[1][:, :, :, :2], args[2])
    with pytest.raises(ValueError):
        eng.unit_backward(args[0][:, :, ::2], args[1], args[2][:, :, ::2])  # strided view
    with pytest.raises(ValueError):
        eng.unit_backward(torch.cat([args[0]] * 2), args[1], torch.cat([args[2]] * 2))  # 4 frames, max_batch 2
    with pytest.raises(ValueError):
        z = torch.zeros((1, 96, 5, 4), device="cuda")
        eng.unit_backward(z, torch.zeros((96, 96, 3, 3), device="cuda"), z)
    with pytest.raises(ValueError):
        z = torch.zeros((1, 64, 1, 1), device="cuda")
        eng.unit_backward(z, args[1], z)
    again = eng.unit_backward(*args, dskip=dev(dskip))
    assert torch.equal(good[0], again[0]) and torch.equal(good[1], again[1])
    # the C ABI's own checks, behind the wrapper's
    rc = eng.lib.pp_unit_backward(eng.ctx, 96, 5, 4, None, None, None, None, 1, None, None, None)
    assert rc != 0
    # the BatchNorm backbone has no unit backward
    bn = load_pkg("engine").Engine(small_cfg(24, 16, 2), norm="batch")
    with pytest.raises(RuntimeError, match="InstanceNorm"):
        bn.unit_backward(*args)
    # taps: before a commit, a wrong canvas, a 16-bit mode
    le, canvas = loaded["eng"], loaded["canvas"]
    base = le.backbone_block_taps(canvas)
    with pytest.raises(RuntimeError):
        eng.backbone_block_taps(torch.zeros((1, 64, 24, 16), device="cuda"))
    with pytest.raises(ValueError):
        le.backbone_block_taps(canvas[:, :-1])
    try:
        le.set_precision("fp16")
        with pytest.raises(RuntimeError, match="fp32"):
            le.backbone_block_taps(canvas)
        w = {k: dev(loaded["sd"][k]) for k in KEYS}
        with pytest.raises(RuntimeError, match="fp32"):
            le.update_block_weights(w)
    finally:
        le.set_precision("fp32")
    # weights: wrong shape / device / missing key; before a commit; another block
    with pytest.raises(ValueError):
        le.update_block_weights({**w, KEYS[1]: w[KEYS[1]][:-1]})
    with pytest.raises(TypeError):
        le.update_block_weights({**w, KEYS[2]: w[KEYS[2]].cpu()})
    with pytest.raises(KeyError):
        le.update_block_weights({k: w[k] for k in KEYS[:-1]})
    with pytest.raises(RuntimeError):
        eng.update_block_weights(w)  # no weights committed
    import ctypes
    ptrs = (ctypes.c_void_p * 5)(*[w[k].data_ptr() for k in KEYS])
    for block, n in ((0, 5), (1, 5), (3, 5), (2, 4)):
        assert le.lib.pp_update_block_weights(le.ctx, block, ptrs, n, None) != 0
        assert b"block 3 only" in le.lib.pp_last_error(le.ctx)
    le.update_block_weights(w)
    assert all(torch.equal(a, b) for a, b in zip(le.backbone_block_taps(canvas), base))
    assert torch.equal(le.backbone(canvas), base[0])  # the hook is inert again
    # the autograd surface in a 16-bit mode, and the BatchNorm network
    net, _ = small_net()
    net.train(scope="block3")
    cv = torch.zeros((1, 64, GX, GY), dtype=torch.float32, device="cuda")
    net.half()
    with pytest.raises(RuntimeError, match="fp32"):
        net.rpn_train(cv)
    net.float()
    assert net.rpn_train(cv).requires_grad
    with pytest.raises(ValueError):
        net.train(scope="block2")
    export = load_pkg("networks.pointpillars8_export")
    cfg = small_cfg(16, 16, 2)
    load_pkg("framework.voxel_generator").VoxelGenerator(cfg)
    with pytest.raises(RuntimeError, match="InstanceNorm"):
        export.PointPillars(cfg).train(scope="block3")
