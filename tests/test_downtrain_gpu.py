"""GPU: the strided stage backward, the tap of block 3's pre-norm conv output and the in-place update of its packed weight
(csrc/down_train.hip, pp_backbone_stage_taps in csrc/conv_run.hip) through the engine wrappers of the C ABI and through the autograd
surface (PointPillars.train(scope="stage3")), against the reference's float64 autograd goldens
(tests/golden/make_downtrain_goldens.py) and the float64 restatement pinned to them (tests/downtrain_ref.py).

Bars.  Fixture gradients: 4 x ref32_dev x max |g64| per tensor, ref32_dev being the reference's own float32-against-float64 deviation
stored in the fixture (the project's bar for gradients).  Everything else: the element-wise a-priori bound of
downtrain_ref.grad_bounds (float32 summation in any order plus the float32 evaluation of dz from float32 inputs).  Equality is
asserted between identical calls, with and without dx, for a frame's dx whatever batch it rides in, between the autograd surface and
the same calls made by hand, and between an engine whose image was rewritten in place and a fresh engine that committed the same
values.  Random conv outputs go through blocktrain_ref.tie_free, so no ReLU argument lies within 1e-4 of zero (asserted)."""
import ctypes
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden, load_pkg
import downtrain_ref as R
from train_common import GX, GY, canvases_of, check_bound, check_grad, dev, small_cfg, small_net, two_frames

sys.path.insert(0, GOLDEN)
from make_downtrain_goldens import DW_STRIDE, MODULES, small_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
KEY = "rpn.block3.0.weight"
_ENGINES = {}


def engine(max_batch=3):
    """An engine without weights (pp_down_backward is stateless and takes its map size from the call)."""
    if max_batch not in _ENGINES:
        load_pkg().install()
        _ENGINES[max_batch] = load_pkg("engine").Engine(small_cfg(24, 16, max_batch))
    return _ENGINES[max_batch]


def seeded_engine(gx, gy):
    load_pkg().install()
    sd = {k: np.asarray(v, np.float32) for k, v in load_pkg("synth").seeded_state_dict(0).items()}
    eng = load_pkg("engine").Engine(small_cfg(gx, gy, 2))
    eng.load_state_dict(sd)
    return eng, sd


def pillar_canvas(gx, gy, seed):
    rng = np.random.default_rng(seed)
    canvas = np.zeros((1, 64, gx, gy), np.float32)
    cells = rng.choice(gx * gy, 300, replace=False)
    canvas[0, :, cells // gy, cells % gy] = np.maximum(rng.standard_normal((300, 64)), 0).astype(np.float32)
    return dev(canvas)


@pytest.fixture(scope="module")
def loaded():
    """48 x 32 cells (level-1 map 12 x 8, level-2 map 6 x 4) with the seeded weights committed and a canvas with a few pillars."""
    eng, sd = seeded_engine(48, 32)
    return dict(eng=eng, sd=sd, canvas=pillar_canvas(48, 32, 3))


def random_case(cin, cout, hin, win, nb, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nb, cin, hin, win)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 3, 3)) * 0.05).astype(np.float32)
    z = R.tie_free(R.conv_s2(x.astype(np.float64), w.astype(np.float64)))
    assert z.dtype == np.float32 and not R.near_ties(z, 1e-4).any()
    dy = rng.standard_normal(z.shape).astype(np.float32)
    return x, w, z, dy


# ------------------------------------------------------------------ 1. fixture gradients
@pytest.mark.parametrize("name", list(MODULES))
def test_fixture_gradients(name):
    g = golden("downtrain_small")
    x, w, dy = small_inputs(name)
    z = g["z_" + name]
    dw, dx = engine().down_backward(dev(x), dev(w), dev(z), dev(dy))
    rdw, rdx = R.down_backward(x, w, z, dy)
    dx_max, dw_max = np.abs(g["dx_" + name]).max(), float(g[f"dw_{name}_max"])
    ddx, ddw = float(g["ref32_dev_dx_" + name]), float(g["ref32_dev_dw_" + name])
    check_grad(dx, g["dx_" + name], ddx, dx_max, f"golden dx {name}")
    check_grad(dx, rdx, ddx, dx_max, f"restated dx {name}")  # every element
    check_grad(dw.reshape(-1)[::DW_STRIDE[name]], g["dw_" + name], ddw, dw_max, f"golden dw {name}")
    check_grad(dw, rdw, ddw, dw_max, f"restated dw {name}")


# ------------------------------------------------------------------ 2. shapes: tile edges, parities, halos, K ranges
@pytest.mark.parametrize("cin,cout,hin,win,nb", [(64, 64, 33, 18, 1), (64, 128, 40, 26, 2), (128, 256, 25, 9, 3), (128, 256, 2, 3, 2),
                                                 (64, 128, 1, 4, 1), (128, 256, 16, 16, 2)])
def test_shapes(cin, cout, hin, win, nb):
    eng = engine()
    x, w, z, dy = random_case(cin, cout, hin, win, nb, 100 + cout + hin)
    xd, wd, zd, dyd = dev(x), dev(w), dev(z), dev(dy)
    dw, dx = eng.down_backward(xd, wd, zd, dyd)
    rw, rx, bw, bx, ties = R.grad_bounds(x, w, z, dy)
    assert not ties.any()
    what = f"{cin}->{cout} {hin}x{win}x{nb}"
    check_bound(dw, rw, bw, what + " dw")
    check_bound(dx, rx, bx, what + " dx")
    dw2, dx2 = eng.down_backward(xd, wd, zd, dyd)
    dw3, none = eng.down_backward(xd, wd, zd, dyd, need_dx=False)
    assert none is None and torch.equal(dw, dw2) and torch.equal(dx, dx2) and torch.equal(dw, dw3)


# ------------------------------------------------------------------ 3. frames
def test_frames():
    eng = engine()
    x, w, z, dy = random_case(64, 128, 13, 10, 2, 7)
    dw, dx = eng.down_backward(dev(x), dev(w), dev(z), dev(dy))
    total = np.zeros(w.shape)
    bound = R.grad_bounds(x, w, z, dy)[2]
    for f in range(2):
        s = slice(f, f + 1)
        dwf, dxf = eng.down_backward(dev(x[s]), dev(w), dev(z[s]), dev(dy[s]))
        assert torch.equal(dxf[0], dx[f]), f  # a frame's dx does not depend on the batch it rides in
        total += dwf.cpu().numpy().astype(np.float64)
        bound = bound + R.grad_bounds(x[s], w, z[s], dy[s])[2]
    check_bound(dw, total, bound, "frames dw")


# ------------------------------------------------------------------ 4. the tap of block 3's conv output
def test_backbone_stage_taps(loaded):
    eng, sd, canvas = loaded["eng"], loaded["sd"], loaded["canvas"]
    want = eng.backbone_block_taps(canvas)
    got = eng.backbone_stage_taps(canvas)
    assert len(got) == 6 and all(torch.equal(a, b) for a, b in zip(got[:5], want))
    assert torch.equal(eng.backbone(canvas), got[0])  # the hook is inert again
    assert all(torch.equal(a, b) for a, b in zip(eng.backbone_block_taps(canvas), want))
    x2, units, z3 = got[2].cpu().numpy(), got[4].cpu().numpy(), got[5].cpu().numpy()
    assert x2.shape == (1, 128, 12, 8) and z3.shape == (1, 256, 6, 4)
    h = np.maximum(R.norm(z3)[0], 0.0)
    err = np.abs(h - units[0:1]).max()
    print(f"relu(norm(z3)) against units[0]: {err:.3e} (max |h| {np.abs(h).max():.3f})")
    assert err <= 2e-4  # the project's backbone bar
    rz = R.conv_s2(x2.astype(np.float64), sd[KEY].astype(np.float64))
    err = np.abs(rz - z3).max()
    print(f"restated conv against z3: {err:.3e} (max |z3| {np.abs(z3).max():.3f})")
    assert err <= 2e-4 and np.abs(z3).max() > 0 and z3.min() < 0  # raw, in front of the norm


# ------------------------------------------------------------------ 5. weight update
def test_update_down_weight():
    UX, UY = 64, 32
    eng, sd = seeded_engine(UX, UY)
    til = eng.layer_tilings()
    print("strided conv of level 2:", [t["tiling"] for t in til if t["kind"] == 0 and t["level"] == 2 and t["stride"] == 2])
    canvas = pillar_canvas(UX, UY, 5)
    rng = np.random.default_rng(6)
    pts = dev(rng.uniform([0, 0, -1.5, 0], [0.2 * UX, 0.2 * UY, 1.0, 1], (6000, 4)).astype(np.float32))
    base = eng.backbone(canvas)
    eng.infer_frame(pts)
    base_rpn = eng.fetch(0, "rpn").clone()
    eng.update_down_weight(2, dev(sd[KEY]))  # the committed values again: the image must not change
    assert torch.equal(eng.backbone(canvas), base)
    eng.infer_frame(pts)
    assert torch.equal(eng.fetch(0, "rpn"), base_rpn)
    new = dict(sd)
    new[KEY] = sd[KEY] + rng.standard_normal(sd[KEY].shape).astype(np.float32) * np.float32(0.02)
    eng.update_down_weight(2, dev(new[KEY]))
    got = eng.backbone(canvas)
    eng.infer_frame(pts)
    got_rpn = eng.fetch(0, "rpn").clone()
    fresh = load_pkg("engine").Engine(small_cfg(UX, UY, 2))  # same shapes: same tilings, same packing, same kernels
    fresh.load_state_dict(new)
    assert fresh.layer_tilings() == til
    assert torch.equal(fresh.backbone(canvas), got)
    fresh.infer_frame(pts)
    assert torch.equal(fresh.fetch(0, "rpn"), got_rpn)
    assert (got - base).abs().max() > 1e-3 and (got_rpn - base_rpn).abs().max() > 1e-3
    eng.update_down_weight(2, dev(sd[KEY]))
    assert torch.equal(eng.backbone(canvas), base)


# ------------------------------------------------------------------ 6 / 7. autograd surface and trajectory
def test_autograd_surface():
    load_pkg().install()
    net, _ = small_net()
    eng = net._eng
    shared = load_pkg("networks.pointpillars8_shared")
    assert eng.DOWN_KEYS == ("rpn.block1.0.weight", "rpn.block2.0.weight", KEY) and shared.STAGE3_KEY == KEY
    example = two_frames(eng)
    plain = net(example)
    net.train(scope="stage3")
    names = [k for k, _ in net.named_parameters()]
    assert names == [KEY] + list(shared.BLOCK3_KEYS + shared.NECK_KEYS + shared.HEAD_KEYS) and len(names) == 15
    assert all(p.is_cuda and p.requires_grad for p in net.parameters())
    preds = net(example)
    for k in plain:
        assert preds[k].requires_grad and torch.equal(preds[k].detach(), plain[k]), k
    rng = np.random.default_rng(8)
    up = {k: dev(rng.standard_normal(tuple(v.shape)).astype(np.float32) * np.float32(1e-2)) for k, v in preds.items()}
    net.zero_grad()
    sum((preds[k] * up[k]).sum() for k in preds).backward()
    params = dict(net.named_parameters())
    grads = {k: p.grad.clone() for k, p in params.items()}
    assert params[KEY].shape == (256, 128, 3, 3)
    # the same chain by hand
    taps = [eng.backbone_stage_taps(c) for c in canvases_of(eng, example)]
    y, x1, x2, x3 = (torch.cat([t[i] for t in taps]) for i in range(4))
    units = [torch.stack([t[4][k] for t in taps]) for k in range(5)]
    z3 = torch.cat([t[5] for t in taps])
    assert torch.equal(y, torch.cat([net.rpn(c) for c in canvases_of(eng, example)]))
    gh, dxh = eng.head_backward(y, up["cls_preds"], up["box_preds"], up["dir_preds"])
    for k in shared.HEAD_KEYS:
        assert torch.equal(grads[k], gh[k].reshape(grads[k].shape)), k
    g = None
    for b, x in enumerate((x1, x2, x3)):
        dw, g = eng.neck_backward(b, x, params[shared.NECK_KEYS[b]].detach(), y, dxh, need_dx=(b == 2))
        assert torch.equal(grads[shared.NECK_KEYS[b]], dw), b
    wb = [params[k].detach() for k in shared.BLOCK3_KEYS]
    h, m3, r3, m4, r4 = units
    dws = [None] * 5
    dws[4], g_r4 = eng.unit_backward(r4, wb[4], g, dskip=g)
    dws[3], g_m4 = eng.unit_backward(m4, wb[3], g_r4)
    dws[2], g_r3 = eng.unit_backward(r3, wb[2], g_m4, dskip=g_r4)
    dws[1], g_m3 = eng.unit_backward(m3, wb[1], g_r3)
    dws[0], g_h = eng.unit_backward(h, wb[0], g_m3, dskip=g_r3, need_du=True)
    for k, key in enumerate(shared.BLOCK3_KEYS):
        assert torch.equal(grads[key], dws[k]), key
    w0 = params[KEY].detach()
    dw0, none = eng.down_backward(x2, w0, z3, g_h, need_dx=False)
    assert none is None and torch.equal(grads[KEY], dw0)
    rw, _, bw, _, ties = R.grad_bounds(x2.cpu().numpy(), w0.cpu().numpy(), z3.cpu().numpy(), g_h.cpu().numpy())
    print(f"stage 3: {int(ties.sum())} near-ties of {ties.size}")
    assert ties.sum() <= 1e-3 * ties.size
    check_bound(dw0, rw, bw, "autograd dw0")
    assert float(dw0.abs().max()) > 0
    # block3 on the same batch: the 14 shared tensors get the same bits
    net.train(scope="block3")
    assert [k for k, _ in net.named_parameters()] == names[1:]
    assert not net._down[KEY].requires_grad
    net.zero_grad()
    preds = net(example)
    sum((preds[k] * up[k]).sum() for k in preds).backward()
    for k, p in net.named_parameters():
        assert torch.equal(p.grad, grads[k]), k
    assert net._down[KEY].grad is None
    net.train()
    assert [k for k, _ in net.named_parameters()] == list(shared.HEAD_KEYS)
    assert not any(p.requires_grad for p in list(net._neck.values()) + list(net._block.values()) + list(net._down.values()))


def test_trajectory():
    """Twenty Adam steps (lr 1e-3, clip_grad_norm_ 10: the reference loop's calls) on a fixed batch of two frames: training the
    stride-2 convolution with block 3, the neck and the head lowers the loss, state_dict() returns the stepped weight, and a fresh
    network loaded with it computes the same backbone output.  The final losses of "stage3" and "block3" are printed side by side;
    which is lower is not asserted."""
    load_pkg().install()
    LossGenerator = load_pkg("framework.loss_generator").LossGenerator
    final = {}
    for scope in ("stage3", "block3"):
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
        if scope == "stage3":
            sd = net.state_dict()
            start = load_pkg("synth").seeded_state_dict(0)
            assert np.abs(sd[KEY] - np.asarray(start[KEY], np.float32).reshape(sd[KEY].shape)).max() > 1e-4  # the stepped weight
            canvas = canvases_of(eng, example)[0]
            want = net.rpn(canvas)
            other, _ = small_net()
            other.load_state_dict(sd)
            assert torch.equal(other.rpn(canvas), want)
    assert final["stage3"][0] == final["block3"][0]
    print("final loss: stage3", final["stage3"][-1], "block3", final["block3"][-1])


# ------------------------------------------------------------------ 8. errors
def test_bad_arguments_raise_and_the_next_call_works(loaded):
    eng = engine(2)
    x, w, z, dy = random_case(64, 128, 5, 4, 2, 1)
    args = [dev(x), dev(w), dev(z), dev(dy)]
    good = eng.down_backward(*args)
    with pytest.raises(TypeError):
        eng.down_backward(args[0].double(), *args[1:])
    with pytest.raises(TypeError):
        eng.down_backward(args[0], args[1].cpu(), args[2], args[3])
    with pytest.raises(TypeError):
        eng.down_backward(args[0], args[1], args[2], dy)
    with pytest.raises(ValueError):
        eng.down_backward(args[0], args[1], args[2][:, :, :, :-1], args[3])
    with pytest.raises(ValueError):
        eng.down_backward(args[0], args[1], args[2], args[3][:, :-1])
    with pytest.raises(ValueError):
        eng.down_backward(args[0], args[1][:, :, :, :2], args[2], args[3])
    with pytest.raises(ValueError):
        eng.down_backward(args[0][:, :, ::2], args[1], args[2][:, :, :2], args[3][:, :, :2])  # strided view
    with pytest.raises(ValueError):
        eng.down_backward(*[torch.cat([t] * 2) if i != 1 else t for i, t in enumerate(args)])  # 4 frames, max_batch 2
    with pytest.raises(ValueError):
        t = torch.zeros((1, 128, 3, 2), device="cuda")  # 128 -> 128 is not a stage of the network
        eng.down_backward(torch.zeros((1, 128, 5, 4), device="cuda"), torch.zeros((128, 128, 3, 3), device="cuda"), t, t)
    with pytest.raises(ValueError):
        t = torch.zeros((1, 128, 1, 1), device="cuda")
        eng.down_backward(torch.zeros((1, 64, 2, 2), device="cuda"), args[1], t, t)  # ho wo = 1
    again = eng.down_backward(*args)
    assert torch.equal(good[0], again[0]) and torch.equal(good[1], again[1])
    # the C ABI's own checks, behind the wrapper's; the next good call works
    p = [ctypes.c_void_p(t.data_ptr()) for t in args]
    out = [ctypes.c_void_p(t.data_ptr()) for t in again]
    lib = eng.lib
    for bad in ((96, 128, 5, 4, 2), (128, 128, 5, 4, 2), (64, 128, 0, 4, 2), (64, 128, 2, 2, 2), (64, 128, 5, 4, 0), (64, 128, 5, 4, 3)):
        assert lib.pp_down_backward(eng.ctx, *bad[:4], *p, bad[4], *out, None) != 0, bad
        assert b"pp_down_backward" in lib.pp_last_error(eng.ctx)
    assert lib.pp_down_backward(eng.ctx, 64, 128, 5, 4, p[0], None, p[2], p[3], 2, *out, None) != 0
    again = eng.down_backward(*args)
    assert torch.equal(good[0], again[0]) and torch.equal(good[1], again[1])
    # the BatchNorm backbone has no stage backward
    bn = load_pkg("engine").Engine(small_cfg(24, 16, 2), norm="batch")
    with pytest.raises(RuntimeError, match="InstanceNorm"):
        bn.down_backward(*args)
    # taps and update: before a commit, a wrong canvas, a 16-bit mode
    le, canvas, w0 = loaded["eng"], loaded["canvas"], dev(loaded["sd"][KEY])
    base = le.backbone_stage_taps(canvas)
    with pytest.raises(RuntimeError):
        eng.backbone_stage_taps(torch.zeros((1, 64, 24, 16), device="cuda"))
    with pytest.raises(RuntimeError):
        eng.update_down_weight(2, w0)  # no weights committed
    with pytest.raises(ValueError):
        le.backbone_stage_taps(canvas[:, :-1])
    try:
        le.set_precision("fp16")
        with pytest.raises(RuntimeError, match="fp32"):
            le.backbone_stage_taps(canvas)
        with pytest.raises(RuntimeError, match="fp32"):
            le.update_down_weight(2, w0)
    finally:
        le.set_precision("fp32")
    # the weight: wrong shape / device; the other levels
    with pytest.raises(ValueError):
        le.update_down_weight(2, w0[:-1])
    with pytest.raises(TypeError):
        le.update_down_weight(2, w0.cpu())
    with pytest.raises(ValueError):
        le.update_down_weight(3, w0)
    with pytest.raises(RuntimeError, match="level 2 only"):
        le.update_down_weight(0, dev(loaded["sd"]["rpn.block1.0.weight"]))
    with pytest.raises(RuntimeError, match="level 2 only"):
        le.update_down_weight(1, dev(loaded["sd"]["rpn.block2.0.weight"]))
    for level in (0, 1, 3):
        assert le.lib.pp_update_down_weight(le.ctx, level, ctypes.c_void_p(w0.data_ptr()), None) != 0
        assert b"level 2 only" in le.lib.pp_last_error(le.ctx)
    le.update_down_weight(2, w0)
    assert all(torch.equal(a, b) for a, b in zip(le.backbone_stage_taps(canvas), base))
    assert torch.equal(le.backbone(canvas), base[0])  # the hook is inert again
    # the autograd surface in a 16-bit mode, and the BatchNorm network
    net, _ = small_net()
    net.train(scope="stage3")
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
        export.PointPillars(cfg).train(scope="stage3")
