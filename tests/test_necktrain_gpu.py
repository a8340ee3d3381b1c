"""GPU: neck backward, backbone taps and the in-place upsampler update (csrc/neck_train.hip) through the engine wrappers of the C ABI
and through the autograd surface (PointPillars.train(scope="neck")), against the reference's float64 autograd goldens
(tests/golden/make_necktrain_goldens.py) and the float64 restatement pinned to them (tests/necktrain_ref.py).

Bars.  Fixture gradients: 4 x ref32_dev x max |g64| per tensor, ref32_dev being the reference's own float32-against-float64 deviation
stored in the fixture (the project's bar for gradients, test_headtrain_gpu.check_grad).  Everything else: the element-wise a-priori
bound of necktrain_ref.grad_bounds (float32 summation in any order plus the float32 evaluation of dZ from a float32 Z).  Equality is
asserted between identical calls, for a frame's dx whatever batch it rides in, and between the autograd surface and the same calls
made by hand."""
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden, load_pkg
import necktrain_ref as R
from train_common import canvases_of, check_bound, check_grad, dev, small_cfg

sys.path.insert(0, GOLDEN)
from make_necktrain_goldens import COFF, CUP, DW_STRIDE, small_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = R.KEYS
_ENGINES = {}


def engine(gx, gy, max_batch=3):
    """An engine without weights (pp_neck_backward is stateless), one per geometry for the whole module."""
    key = (gx, gy, max_batch)
    if key not in _ENGINES:
        load_pkg().install()
        _ENGINES[key] = load_pkg("engine").Engine(small_cfg(gx, gy, max_batch))
    return _ENGINES[key]


@pytest.fixture(scope="module")
def loaded():
    """12 x 8 map with the seeded weights committed, a canvas with a few pillars and its backbone output."""
    load_pkg().install()
    synth = load_pkg("synth")
    eng = load_pkg("engine").Engine(small_cfg(24, 16, 2))
    sd = {k: np.asarray(v, np.float32) for k, v in synth.seeded_state_dict(0).items()}
    eng.load_state_dict(sd)
    rng = np.random.default_rng(3)
    canvas = np.zeros((1, 64, 24, 16), np.float32)
    cells = rng.choice(24 * 16, 90, replace=False)
    canvas[0, :, cells // 16, cells % 16] = np.maximum(rng.standard_normal((90, 64)), 0).astype(np.float32)
    canvas = dev(canvas)
    return dict(eng=eng, sd=sd, canvas=canvas, rpn=eng.backbone(canvas))


def random_case(H, W, nb, seed):
    """x_k, w_k, y (the float32 cast of the float64 forward) and dy for a level-0 map H x W."""
    rng = np.random.default_rng(seed)
    xs = [rng.standard_normal((nb, R.CIN[b], H >> b, W >> b)).astype(np.float32) for b in range(3)]
    ws = [(rng.standard_normal((R.CIN[b], R.CUP[b], 1 << b, 1 << b)) * 0.05).astype(np.float32) for b in range(3)]
    y = np.concatenate([R.branch_forward(xs[b], ws[b]) for b in range(3)], 1).astype(np.float32)
    dy = rng.standard_normal((nb, 320, H, W)).astype(np.float32)
    return xs, ws, y, dy


# ------------------------------------------------------------------ 1. fixture gradients
def test_fixture_gradients():
    g = golden("necktrain_small")
    xs, ws, dy = small_inputs()
    eng = engine(24, 16, 2)
    y = g["y"]
    for b in range(3):
        sl = slice(COFF[b], COFF[b] + CUP[b])
        dw, dx = eng.neck_backward(b, dev(xs[b]), dev(ws[b]), dev(y), dev(dy))
        n = f"{b + 1}"
        dw_max = float(g["dw" + n + "_max"])
        check_grad(dx, g["dx" + n], float(g["ref32_dev_dx" + n]), np.abs(g["dx" + n]).max(), "golden dx" + n)
        samples = dw.reshape(-1)[::DW_STRIDE[b]] if DW_STRIDE[b] > 1 else dw
        check_grad(samples, g["dw" + n], float(g["ref32_dev_dw" + n]), dw_max, "golden dw" + n)
        rw, rx = R.branch_backward(xs[b], ws[b], y[:, sl], dy[:, sl])  # every element, against the restatement the CPU test pins
        check_grad(dw, rw, float(g["ref32_dev_dw" + n]), dw_max, "restated dw" + n)
        check_grad(dx, rx, float(g["ref32_dev_dx" + n]), np.abs(g["dx" + n]).max(), "restated dx" + n)


# ------------------------------------------------------------------ 2. medium maps
@pytest.mark.parametrize("H,W,nb", [(40, 24, 3), (20, 36, 1)])
def test_medium_maps(H, W, nb):
    eng = engine(2 * H, 2 * W)
    xs, ws, y, dy = random_case(H, W, nb, 100 + H)
    yd, dyd = dev(y), dev(dy)
    for b in range(3):
        sl = slice(R.COFF[b], R.COFF[b] + R.CUP[b])
        xd, wd = dev(xs[b]), dev(ws[b])
        dw, dx = eng.neck_backward(b, xd, wd, yd, dyd)
        rw, rx, bw, bx = R.grad_bounds(xs[b], ws[b], y[:, sl], dy[:, sl])
        check_bound(dw, rw, bw, f"{H}x{W} dw{b + 1}")
        check_bound(dx, rx, bx, f"{H}x{W} dx{b + 1}")
        dw2, dx2 = eng.neck_backward(b, xd, wd, yd, dyd)
        dw3, none = eng.neck_backward(b, xd, wd, yd, dyd, need_dx=False)
        assert none is None and torch.equal(dw, dw2) and torch.equal(dx, dx2) and torch.equal(dw, dw3), b


# ------------------------------------------------------------------ 3. frames
def test_frames():
    H, W, nb = 40, 24, 2
    eng = engine(2 * H, 2 * W)
    xs, ws, y, dy = random_case(H, W, nb, 7)
    for b in range(3):
        sl = slice(R.COFF[b], R.COFF[b] + R.CUP[b])
        dw, dx = eng.neck_backward(b, dev(xs[b]), dev(ws[b]), dev(y), dev(dy))
        total = np.zeros(ws[b].shape)
        bound = R.grad_bounds(xs[b], ws[b], y[:, sl], dy[:, sl])[2]
        for f in range(nb):
            dwf, dxf = eng.neck_backward(b, dev(xs[b][f:f + 1]), dev(ws[b]), dev(y[f:f + 1]), dev(dy[f:f + 1]))
            assert torch.equal(dxf[0], dx[f]), (b, f)  # a frame's dx does not depend on the batch it rides in
            total += dwf.cpu().numpy().astype(np.float64)
            bound = bound + R.grad_bounds(xs[b][f:f + 1], ws[b], y[f:f + 1, sl], dy[f:f + 1, sl])[2]
        check_bound(dw, total, bound, f"frames dw{b + 1}")


# ------------------------------------------------------------------ 4. backbone taps
def test_backbone_taps(loaded):
    eng, sd = loaded["eng"], loaded["sd"]
    rpn, x1, x2, x3 = eng.backbone_taps(loaded["canvas"])
    assert torch.equal(rpn, loaded["rpn"]) and torch.equal(eng.backbone(loaded["canvas"]), rpn)
    want = rpn.cpu().numpy()
    for b, x in enumerate((x1, x2, x3)):
        assert tuple(x.shape) == (1,) + eng.neck_shapes(b)[0]
        y = R.branch_forward(x.cpu().numpy(), sd[KEYS[b]])
        err = np.abs(y - want[:, R.COFF[b]:R.COFF[b] + R.CUP[b]]).max()
        print(f"tap {b + 1}: restated forward against rpn_out {err:.3e}")
        assert err <= 2e-4, b  # the project's backbone bar


# ------------------------------------------------------------------ 5. weight update
def test_update_neck_weights(loaded):
    eng, sd, canvas, base = loaded["eng"], loaded["sd"], loaded["canvas"], loaded["rpn"]
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.uniform([0, 0, -1.5, 0], [4.8, 3.2, 1.0, 1], (4000, 4))]).astype(np.float32)
    pts = dev(pts)
    new = dict(sd)
    for k in KEYS:
        new[k] = sd[k] + rng.standard_normal(sd[k].shape).astype(np.float32) * np.float32(0.02)
    try:
        eng.update_neck_weights({k: dev(sd[k]) for k in KEYS})  # the committed values again: the images must not change
        assert torch.equal(eng.backbone(canvas), base)
        eng.infer_frame(pts)
        old_rpn = eng.fetch(0, "rpn").clone()
        eng.update_neck_weights({k: dev(new[k]) for k in KEYS})
        got = eng.backbone(canvas)
        eng.infer_frame(pts)
        got_rpn = eng.fetch(0, "rpn").clone()
        fresh = load_pkg("engine").Engine(small_cfg(24, 16, 2))  # same shapes: same tilings, same packing, same kernels
        fresh.load_state_dict(new)
        assert fresh.layer_tilings() == eng.layer_tilings()
        assert torch.equal(fresh.backbone(canvas), got)
        fresh.infer_frame(pts)
        assert torch.equal(fresh.fetch(0, "rpn"), got_rpn)
        assert (got - base).abs().max() > 1e-3 and (got_rpn - old_rpn).abs().max() > 1e-3
    finally:
        eng.update_neck_weights({k: dev(sd[k]) for k in KEYS})
    assert torch.equal(eng.backbone(canvas), base)


# ------------------------------------------------------------------ 6 / 7. autograd surface and trajectory
def small_net(seed=0):
    cfg = small_cfg(16, 16, 4)
    load_pkg("framework.voxel_generator").VoxelGenerator(cfg)
    net = load_pkg("networks.pointpillars8_shared").PointPillars(cfg)
    net.load_state_dict(load_pkg("synth").seeded_state_dict(seed))
    return net, cfg


def two_frames(eng):
    rng = np.random.default_rng(4)
    frames = []
    for f in range(2):
        n = 30 + 10 * f
        cells = rng.choice(16 * 16, n, replace=False)
        coors = np.stack([cells // 16, cells % 16, np.zeros(n, np.int64)], 1).astype(np.int32)
        vox = rng.standard_normal((n, eng.T, eng.F)).astype(np.float32)
        frames.append(dict(voxels=vox, coordinates=coors, num_points_per_voxel=rng.integers(1, eng.T + 1, n).astype(np.int32)))
    utils = load_pkg("framework.utils")
    return utils.example_convert_to_torch(utils.merge_second_batch(frames))


def test_autograd_surface():
    load_pkg().install()
    net, _ = small_net()
    eng = net._eng
    shared = load_pkg("networks.pointpillars8_shared")
    example = two_frames(eng)
    plain = net(example)
    assert all(v.grad_fn is None for v in plain.values())
    net.train(scope="neck")
    names = [k for k, _ in net.named_parameters()]
    assert names == list(shared.NECK_KEYS + shared.HEAD_KEYS) and all(p.is_cuda and p.requires_grad for p in net.parameters())
    preds = net(example)
    for k in plain:
        assert preds[k].requires_grad and torch.equal(preds[k].detach(), plain[k]), k
    rng = np.random.default_rng(8)
    up = {k: dev(rng.standard_normal(tuple(v.shape)).astype(np.float32) * np.float32(1e-2)) for k, v in preds.items()}
    net.zero_grad()
    sum((preds[k] * up[k]).sum() for k in preds).backward()
    # the same by hand
    taps = [eng.backbone_taps(c) for c in canvases_of(eng, example)]
    y, x1, x2, x3 = (torch.cat([t[i] for t in taps]) for i in range(4))
    assert torch.equal(y, net.rpn_train(torch.cat(canvases_of(eng, example))).detach())
    gh, dxh = eng.head_backward(y, up["cls_preds"], up["box_preds"], up["dir_preds"])
    params = dict(net.named_parameters())
    for k in shared.HEAD_KEYS:
        assert torch.equal(params[k].grad, gh[k].reshape(params[k].shape)), k
    for b, x in enumerate((x1, x2, x3)):
        p = params[KEYS[b]]
        dw, none = eng.neck_backward(b, x, p.detach(), y, dxh, need_dx=False)
        assert none is None and p.grad is not None and torch.equal(p.grad, dw), b
        sl = slice(R.COFF[b], R.COFF[b] + R.CUP[b])
        rw, _, bw, _ = R.grad_bounds(x.cpu().numpy(), p.detach().cpu().numpy(), y[:, sl].cpu().numpy(), dxh[:, sl].cpu().numpy())
        check_bound(p.grad, rw, bw, f"autograd dw{b + 1}")
    net.train()
    assert [k for k, _ in net.named_parameters()] == list(shared.HEAD_KEYS)
    assert not any(p.requires_grad for p in net._neck.values())


def test_trajectory():
    """Twenty Adam steps (lr 1e-3, clip_grad_norm_ 10: the reference loop's calls) on a fixed batch of two frames: training the neck
    with the head lowers the loss, and lowers it further than the head alone from the same start."""
    load_pkg().install()
    LossGenerator = load_pkg("framework.loss_generator").LossGenerator
    final = {}
    for scope in ("neck", "head"):
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
        if scope == "neck":
            sd = net.state_dict()
            start = load_pkg("synth").seeded_state_dict(0)
            for k in KEYS:  # state_dict returns the stepped upsamplers
                assert np.abs(sd[k] - np.asarray(start[k], np.float32).reshape(sd[k].shape)).max() > 1e-4, k
    assert final["neck"][0] == final["head"][0]
    assert final["neck"][-1] < final["head"][-1], final


# ------------------------------------------------------------------ 8. errors
def test_bad_arguments_raise_and_the_next_call_works(loaded):
    eng = engine(24, 16, 2)
    xs, ws, dy = small_inputs()
    y = golden("necktrain_small")["y"]
    args = [dev(xs[1]), dev(ws[1]), dev(y), dev(dy)]
    good = eng.neck_backward(1, *args)
    with pytest.raises(TypeError):
        eng.neck_backward(1, args[0].double(), *args[1:])
    with pytest.raises(TypeError):
        eng.neck_backward(1, args[0], args[1].cpu(), *args[2:])
    with pytest.raises(ValueError):
        eng.neck_backward(1, args[0][:, :, :, :-1], *args[1:])
    with pytest.raises(ValueError):
        eng.neck_backward(1, args[0], args[1], args[2][:, :-1], args[3])
    with pytest.raises(ValueError):
        eng.neck_backward(1, torch.cat([args[0]] * 2), args[1], torch.cat([args[2]] * 2), torch.cat([args[3]] * 2))  # 4 frames, max_batch 2
    with pytest.raises(ValueError):
        eng.neck_backward(3, *args)
    with pytest.raises(ValueError):
        eng.neck_backward(0, *args)  # branch 1's tensors
    again = eng.neck_backward(1, *args)
    assert torch.equal(good[0], again[0]) and torch.equal(good[1], again[1])
    # the BatchNorm backbone has no neck backward
    bn = load_pkg("engine").Engine(small_cfg(24, 16, 2), norm="batch")
    with pytest.raises(RuntimeError, match="InstanceNorm"):
        bn.neck_backward(1, *args)
    # weights: wrong shape / device / missing key; before a commit
    le, sd, canvas = loaded["eng"], loaded["sd"], loaded["canvas"]
    w = {k: dev(sd[k]) for k in KEYS}
    with pytest.raises(ValueError):
        le.update_neck_weights({**w, KEYS[1]: w[KEYS[1]][:-1]})
    with pytest.raises(TypeError):
        le.update_neck_weights({**w, KEYS[2]: w[KEYS[2]].cpu()})
    with pytest.raises(KeyError):
        le.update_neck_weights({k: w[k] for k in KEYS[:-1]})
    with pytest.raises(RuntimeError):
        eng.update_neck_weights(w)  # no weights committed
    with pytest.raises(RuntimeError):
        eng.backbone_taps(canvas)
    with pytest.raises(ValueError):
        le.backbone_taps(canvas[:, :-1])
    # a 16-bit mode
    try:
        le.set_precision("fp16")
        with pytest.raises(RuntimeError, match="fp32"):
            le.update_neck_weights(w)
        with pytest.raises(RuntimeError, match="fp32"):
            le.backbone_taps(canvas)
    finally:
        le.set_precision("fp32")
    taps = le.backbone_taps(canvas)
    assert torch.equal(taps[0], loaded["rpn"])
    # the autograd surface in a 16-bit mode
    net, _ = small_net()
    net.train(scope="neck")
    cv = torch.zeros((1, 64, 16, 16), dtype=torch.float32, device="cuda")
    net.half()
    with pytest.raises(RuntimeError, match="fp32"):
        net.rpn_train(cv)
    net.float()
    assert net.rpn_train(cv).requires_grad
    export = load_pkg("networks.pointpillars8_export")
    cfg = small_cfg(16, 16, 2)
    load_pkg("framework.voxel_generator").VoxelGenerator(cfg)
    with pytest.raises(RuntimeError, match="InstanceNorm"):
        export.PointPillars(cfg).train(scope="neck")
