"""GPU: training the whole RPN -- the taps of every level (pp_backbone_train_taps), the in-place update of all sixteen packed
convolution images and of the sparse first convolution's image (pp_update_rpn_weights) and the autograd surface
PointPillars.train(scope="rpn") -- against the reference's float64 autograd goldens (tests/golden/make_rpntrain_goldens.py) and the
float64 restatement pinned to them (tests/rpntrain_ref.py).

Bars.  Fixture gradients: 4 x ref32_dev x max |g64| per tensor, ref32_dev being the reference's own float32-against-float64 deviation
stored in the fixture (train_common.check_grad).  Per-convolution gradients of the autograd surface: the element-wise a-priori
bounds of blocktrain_ref.grad_bounds / downtrain_ref.grad_bounds, evaluated from the GPU's own taps.  Taps: the backbone's bar of 2e-4
against the float64 restatement of the forward (the CPU oracle of the intermediate tensors; oracle/pp_oracle.py hands out rpn_out
only, which is compared as well).  Equality is asserted between the tap entry points, between the autograd surface and the same chain
made by hand with the engine primitives, between scopes on the tensors they share, and between an engine whose images were rewritten
in place and a fresh engine that committed the same values: image by image (pp_weight_image), through backbone() and through the
fused pass pp_infer_frame, which is the pass that runs the sparse first convolution and tile skipping."""
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden, load_pkg
import rpntrain_ref as R
from train_common import (GX, GY, by_hand, canvases_of, check_bound, check_grad, dev, loaded, seeded_sd, small_cfg, small_net,  # noqa: F401
                          stacked_taps, two_frames)

sys.path.insert(0, GOLDEN)
from make_rpntrain_goldens import DW_STRIDE, DX_STRIDE, small_inputs, split  # noqa: E402

pytestmark = pytest.mark.gpu
ENG = load_pkg("engine").Engine
CONV, NECK = ENG.RPN_CONV_KEYS, ENG.NECK_KEYS
BAR = 2e-4  # the project's backbone bar


# ------------------------------------------------------------------ 1. taps
def test_backbone_train_taps(loaded):  # noqa: F811
    eng, sd, canvas = loaded["eng"], loaded["sd"], loaded["canvas"]
    want = eng.backbone_taps(canvas)
    stage = eng.backbone_stage_taps(canvas)
    y, xs, units, zs = eng.backbone_train_taps(canvas)
    assert torch.equal(y, want[0]) and all(torch.equal(a, b) for a, b in zip(xs, want[1:]))
    assert torch.equal(units[2], stage[4]) and torch.equal(zs[2], stage[5])
    fwd = R.rpn_forward(canvas.cpu().numpy(), [sd[k] for k in CONV], [sd[k] for k in NECK])
    for b in range(3):
        shape = (64 << b, 24 >> b, 16 >> b)
        assert units[b].shape == (ENG.RPN_UNITS[b],) + shape and zs[b].shape == (1,) + shape and xs[b].shape == (1,) + shape
        u, z = units[b].cpu().numpy().astype(np.float64), zs[b].cpu().numpy()
        h = np.maximum(R.B.norm(z)[0], 0.0)
        err = np.abs(h[0] - u[0]).max()
        print(f"level {b}: units[0] against relu(norm(z)) {err:.3e}")
        assert err <= BAR and u[0].min() >= 0 and u[0].max() > 0, b
        pairs = [("z", z, fwd["zs"][b]), ("x", xs[b].cpu().numpy(), fwd["taps"][b])] + \
                [(f"unit {k}", u[k:k + 1], fwd["units"][b][k]) for k in range(ENG.RPN_UNITS[b])]
        for name, got, ref in pairs:
            err = np.abs(got - ref).max()
            print(f"level {b} {name}: against the float64 forward {err:.3e} (max |tap| {np.abs(ref).max():.3f})")
            assert err <= BAR, (b, name)
    assert np.abs(y.cpu().numpy() - fwd["y"]).max() <= BAR
    from oracle import pp_oracle as O
    assert np.abs(y.cpu().numpy() - O.backbone(canvas.cpu().numpy(), sd)).max() <= BAR
    assert torch.equal(eng.backbone(canvas), want[0])  # the hooks are inert again
    assert all(torch.equal(a, b) for a, b in zip(eng.backbone_stage_taps(canvas), stage))


# ------------------------------------------------------------------ 2. weight update
UX, UY = 64, 32  # cells: the level-2 map is 8 x 4, whole 4 x 4 tiles, so that wino6 can be forced too


def images(eng):
    til = eng.layer_tilings()
    conv = [i for i, t in enumerate(til) if t["kind"] == 0]
    assert len(conv) == 16
    return [eng.weight_image(i).clone() for i in conv] + [eng.weight_image(-1).clone()]


def perturbed(sd, rng):
    new = dict(sd)
    for k in CONV:
        new[k] = sd[k] + rng.standard_normal(sd[k].shape).astype(np.float32) * np.float32(0.02)
    return new


@pytest.mark.parametrize("force", [None, "wino6 tw4", "wino4 tw4 bx2", "wino tw8", "k3s1 tw8 w2x2 t4x5"])
def test_update_rpn_weights(force, monkeypatch):
    if force:
        monkeypatch.setenv("PP_FORCE_VARIANT", force)  # ahead of the engines: the tuner reads it at commit time
    load_pkg().install()
    sd = seeded_sd()
    eng = ENG(small_cfg(UX, UY, 2))
    eng.load_state_dict(sd)
    til = eng.layer_tilings()
    s1 = [t["tiling"] for t in til if t["kind"] == 0 and t["stride"] == 1]
    print(force, s1)
    assert len(s1) == 13 and (force is None or sum(force in t for t in s1) >= 5)
    rng = np.random.default_rng(5)
    canvas = np.zeros((1, 64, UX, UY), np.float32)
    cells = rng.choice(UX * UY, 300, replace=False)
    canvas[0, :, cells // UY, cells % UY] = np.maximum(rng.standard_normal((300, 64)), 0).astype(np.float32)
    canvas = dev(canvas)
    new = perturbed(sd, rng)
    fresh = ENG(small_cfg(UX, UY, 2))  # same shapes: same tilings, same packing, same kernels
    fresh.load_state_dict(new)
    assert fresh.layer_tilings() == til
    want = {"old": (images(eng), eng.backbone(canvas)), "new": (images(fresh), fresh.backbone(canvas))}
    assert (want["old"][1] - want["new"][1]).abs().max() > 1e-3
    assert not any(torch.equal(a, b) for a, b in zip(*[want[k][0] for k in ("old", "new")]))
    for which, vals in (("old", sd), ("new", new), ("old", sd)):  # the committed values, perturbed ones, and back
        eng.update_rpn_weights({k: dev(vals[k]) for k in CONV})
        got = images(eng)
        for i, (a, b) in enumerate(zip(got, want[which][0])):
            assert a.shape == b.shape and torch.equal(a, b), (which, "sparse first conv" if i == 16 else til[i]["tiling"])
        assert torch.equal(eng.backbone(canvas), want[which][1]), which


def test_the_three_updaters_share_their_image_maps():
    """pp_update_down_weight, pp_update_rpn_weights and pp_update_block_weights write through one cache of position maps, filled
    entry by entry and dropped by a commit: narrow and whole updates in turn, a commit in between (two changes of precision mode),
    narrow updates again -- and every packed image, with the sparse first convolution's, is the one a fresh engine packs from the
    values that went up last."""
    load_pkg().install()
    sd = seeded_sd()
    eng = ENG(small_cfg(UX, UY, 2))
    eng.load_state_dict(sd)
    rng = np.random.default_rng(11)
    down, block = ENG.DOWN_KEYS[2], ENG.BLOCK3_KEYS
    a, b, c, d = (perturbed(sd, rng) for _ in range(4))
    eng.update_down_weight(2, dev(a[down]))  # fills entry 10 only
    eng.update_rpn_weights({k: dev(b[k]) for k in CONV})  # the other fifteen
    eng.update_block_weights({k: dev(c[k]) for k in block})
    final = dict(b, **{k: c[k] for k in block})
    fresh = ENG(small_cfg(UX, UY, 2))
    fresh.load_state_dict(final)
    assert fresh.layer_tilings() == eng.layer_tilings()
    for i, (got, want) in enumerate(zip(images(eng), images(fresh))):
        assert got.shape == want.shape and torch.equal(got, want), ("before the commit", i)
    eng.set_precision("bf16x3")
    eng.set_precision("fp32")  # commits sd again: every map is stale, and the images hold sd's values
    eng.update_block_weights({k: dev(d[k]) for k in block})
    eng.update_down_weight(2, dev(d[down]))
    final = dict(sd, **{k: d[k] for k in block + (down,)})
    fresh.load_state_dict(final)
    assert fresh.layer_tilings() == eng.layer_tilings()
    for i, (got, want) in enumerate(zip(images(eng), images(fresh))):
        assert got.shape == want.shape and torch.equal(got, want), ("after the commit", i)


TX, TY = 128, 160  # cells: the level-0 map is 64 x 80 = 4 x 5 tiles of 16 x 16, the geometry of test_tile_skip_gpu.py


@pytest.mark.parametrize("kc", [4, 8])
def test_update_reaches_the_fused_pass(kc, monkeypatch):
    """The fused pass (pp_infer_frame: sparse first convolution, tile skipping at level 0) after an in-place update, against a fresh
    network that loaded the same values; the first convolution's tiling is pinned to `kc` channels per chunk, whose K order the sparse
    kernel's image follows, and level 0 to wino6, which tile skipping needs."""
    monkeypatch.setenv("PP_FORCE_VARIANT", f"wino6;k3s2 tw16 w1x4 t4x5 bx1 kc{kc}")
    load_pkg().install()
    shared = load_pkg("networks.pointpillars8_shared")

    def make():
        cfg = small_cfg(TX, TY, 2)
        cfg["max_voxels"] = 4000
        load_pkg("framework.voxel_generator").VoxelGenerator(cfg)
        net = shared.PointPillars(cfg)
        net.load_state_dict(load_pkg("synth").seeded_state_dict(0))
        net.profile_stages = False
        return net

    def fused(net, pts, example):
        eng = net._eng
        eng.set_sparse_conv1(True)
        eng.set_tile_skip(True)
        with torch.no_grad():
            preds = net(example)  # syncs the stepped weights into the engine
        det, cnt = eng.infer_frame(pts)
        torch.cuda.synchronize()
        assert eng.tile_skip_active()
        flags = eng.fetch(0, "tile_flags").cpu().numpy()
        assert flags.any() and not flags.all()  # some tiles were skipped, some computed
        assert int(eng.fetch(0, "active")[0]) > 0  # the sparse first convolution ran
        return preds, eng.fetch(0, "rpn").clone(), det.clone(), cnt.clone()

    net = make()
    til = net._eng.layer_tilings()
    assert f"kc{kc} " in til[0]["tiling"] and all(til[i]["wino"] == 6 for i in (1, 2, 3)), [t["tiling"] for t in til[:4]]
    rng = np.random.default_rng(9)
    pts = dev(rng.uniform([8.0, 10.0, -1.5, 0], [14.0, 17.0, 1.0, 1], (4000, 4)).astype(np.float32))
    v, c, n, num = net._eng.voxelize(pts)
    k = int(num.item())
    example = {"voxels": v[:k].contiguous(), "coordinates": c[:k].contiguous(), "num_points_per_voxel": n[:k].contiguous()}
    base = fused(net, pts, example)
    net.train(scope="rpn")
    with torch.no_grad():
        for key, p in net.named_parameters():
            if key in CONV:
                p.add_(dev(rng.standard_normal(tuple(p.shape)).astype(np.float32) * np.float32(0.02)))
    net.eval()
    got = fused(net, pts, example)
    assert (got[1] - base[1]).abs().max() > 1e-3
    other = make()
    other.load_state_dict(net.state_dict())
    assert other._eng.layer_tilings() == til
    want = fused(other, pts, example)
    for key in want[0]:
        assert torch.equal(got[0][key], want[0][key]), key
    assert all(torch.equal(a, b) for a, b in zip(got[1:], want[1:]))
    for a, b in zip(images(net._eng), images(other._eng)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 3. autograd surface
def test_autograd_surface():
    load_pkg().install()
    net, _ = small_net()
    eng = net._eng
    shared = load_pkg("networks.pointpillars8_shared")
    example = two_frames(eng)
    plain = net(example)
    assert all(v.grad_fn is None for v in plain.values())
    rng = np.random.default_rng(8)
    up = {k: dev(rng.standard_normal(tuple(v.shape)).astype(np.float32) * np.float32(1e-2)) for k, v in plain.items()}
    grads = {}
    for scope in ("neck", "block3", "stage3", "rpn"):
        net.train(scope=scope)
        preds = net(example)
        for k in plain:
            assert preds[k].requires_grad and torch.equal(preds[k].detach(), plain[k]), (scope, k)  # the inference bits
        net.zero_grad()
        sum((preds[k] * up[k]).sum() for k in preds).backward()
        grads[scope] = {k: p.grad.clone() for k, p in net.named_parameters()}
    names = [k for k, _ in net.named_parameters()]
    assert names == list(shared.RPN_KEYS) and len(names) == 25
    assert all(p.is_cuda and p.requires_grad for p in net.parameters())
    assert [len(grads[scope]) for scope in ("neck", "block3", "stage3", "rpn")] == [9, 14, 15, 25]
    for scope in ("neck", "block3", "stage3"):  # the tensors a narrower scope trains get the same bits as under "rpn"
        for k, g in grads[scope].items():
            assert torch.equal(g, grads["rpn"][k]), (scope, k)
    # the same chain by hand
    frames = canvases_of(eng, example)
    canvases = torch.cat(frames)
    taps = stacked_taps(eng, frames)
    y = taps[0]
    assert torch.equal(y, net.rpn_train(canvases).detach()) and torch.equal(y, torch.cat([net.rpn(c) for c in frames]))
    gh, dxh = eng.head_backward(y, up["cls_preds"], up["box_preds"], up["dir_preds"])
    p = {k: v.detach() for k, v in net.named_parameters()}
    for k in shared.HEAD_KEYS:
        assert torch.equal(grads["rpn"][k], gh[k].reshape(p[k].shape)), k
    dw, dcanvas, seen = by_hand(eng, canvases, taps, p, dxh, need_dx=True)
    assert sorted(dw) == sorted(CONV + NECK)
    for k in CONV + NECK:
        assert torch.equal(grads["rpn"][k], dw[k]), k
    # every convolution's dw within its a-priori bound, evaluated from the GPU's own taps
    for k in CONV:
        args = [t.cpu().numpy() for t in seen[k]]
        if len(args) == 2:
            rw, _, bw, _, ties = R.B.grad_bounds(args[0], p[k].cpu().numpy(), args[1])
        else:
            rw, _, bw, _, ties = R.D.grad_bounds(args[0], p[k].cpu().numpy(), args[1], args[2])
        print(f"{k}: {int(ties.sum())} near-ties of {ties.size}")
        assert ties.sum() <= 1e-3 * ties.size, k
        check_bound(grads["rpn"][k], rw, bw, f"autograd dw {k}")
    # the canvases' gradient: level 0's dx when, and only when, they require grad
    net.zero_grad()
    cv = canvases.clone().requires_grad_()
    out = net.rpn_train(cv)
    assert torch.equal(out.detach(), y)
    out.backward(dxh)
    assert cv.grad is not None and torch.equal(cv.grad, dcanvas) and float(cv.grad.abs().max()) > 0
    for k in CONV + NECK:
        assert torch.equal(dict(net.named_parameters())[k].grad, dw[k]), k
    cv2 = canvases.clone()
    net.rpn_train(cv2).backward(dxh)
    assert cv2.grad is None
    net.train()
    assert [k for k, _ in net.named_parameters()] == list(shared.HEAD_KEYS)
    assert not any(q.requires_grad for d in (net._neck, net._block, net._down, net._rpn) for q in d.values())


# ------------------------------------------------------------------ 4. the fixture through the Function
def test_fixture_chain():
    """The fixture's canvases, weights and dy through _RpnFunction against the reference's float64 gradients.  A ReLU that takes
    another branch on the GPU than in float64 changes a gradient by a jump no tolerance describes, so the masks are compared first."""
    load_pkg().install()
    g = golden("rpntrain_small")
    canvas, ws, dy = small_inputs()
    wc, wn = split(ws)
    cfg = small_cfg(canvas.shape[2], canvas.shape[3], 2)
    load_pkg("framework.voxel_generator").VoxelGenerator(cfg)
    net = load_pkg("networks.pointpillars8_shared").PointPillars(cfg)
    sd = seeded_sd()
    for k, w in zip(R.KEYS, ws):
        assert sd[k].shape == w.shape, k
        sd[k] = w
    net.load_state_dict(sd)
    eng = net._eng
    cv = dev(canvas)
    y, xs, units, zs = stacked_taps(eng, cv)
    fwd = R.rpn_forward(canvas, wc, wn)
    want = R.relu_masks(fwd["y"], fwd["units"], fwd["zs"])
    got = R.relu_masks(y.cpu().numpy(), [[u.cpu().numpy() for u in us] for us in units], [z.cpu().numpy() for z in zs])
    for site in want:
        flipped = int((want[site] != got[site]).sum())
        assert flipped == 0, f"ReLU mask flipped at {site}: {flipped} of {want[site].size} elements take another branch on the GPU than in float64"
    net.train(scope="rpn")
    cvg = cv.clone().requires_grad_()
    out = net.rpn_train(cvg)
    assert np.abs(out.detach().cpu().numpy() - fwd["y"]).max() <= BAR
    out.backward(dev(dy))
    params = dict(net.named_parameters())
    for i, k in enumerate(R.KEYS):
        check_grad(params[k].grad.reshape(-1)[::DW_STRIDE], g[f"dw_{i}"], float(g[f"ref32_dev_dw_{i}"]), float(g[f"dw_{i}_max"]), f"golden dw {k}")
    check_grad(cvg.grad.reshape(-1)[::DX_STRIDE], g["dcanvas"], float(g["ref32_dev_dcanvas"]), float(g["dcanvas_max"]), "golden dcanvas")


# ------------------------------------------------------------------ 5. trajectory
def test_trajectory():
    """Twenty Adam steps (lr 1e-3, clip_grad_norm_ 10: the reference loop's calls) on a fixed batch of two frames: training the whole
    RPN lowers the loss, state_dict() returns the stepped weights of blocks 1 and 2 and of a strided convolution, and a fresh network
    loaded with it computes the same backbone output, the same predictions and the same fused pass.  The final losses of "rpn" and
    "stage3" are printed side by side; which is lower is not asserted."""
    load_pkg().install()
    LossGenerator = load_pkg("framework.loss_generator").LossGenerator
    final = {}
    for scope in ("rpn", "stage3"):
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
        if scope == "rpn":
            sd = net.state_dict()
            start = load_pkg("synth").seeded_state_dict(0)
            for k in ("rpn.block1.3.conv_block.5.weight", "rpn.block2.4.conv_block.2.weight", "rpn.block1.0.weight", "rpn.block2.0.weight"):
                assert np.abs(sd[k] - np.asarray(start[k], np.float32).reshape(sd[k].shape)).max() > 1e-4, k
            canvas = canvases_of(eng, example)[0]
            pts = dev(rng.uniform([0, 0, -1.5, 0], [0.2 * GX, 0.2 * GY, 1.0, 1], (3000, 4)).astype(np.float32))
            net.eval()
            other, _ = small_net()
            other.load_state_dict(sd)
            assert torch.equal(other.rpn(canvas), net.rpn(canvas))
            pa, pb = net(example), other(example)
            assert all(torch.equal(pa[k], pb[k]) for k in pa)
            da, db = eng.infer_frame(pts), other._eng.infer_frame(pts)  # the fused pass: it reads the sparse first convolution's image
            assert torch.equal(eng.fetch(0, "rpn"), other._eng.fetch(0, "rpn")) and all(torch.equal(x, y) for x, y in zip(da, db))
    assert final["rpn"][0] == final["stage3"][0]
    print("final loss: rpn", final["rpn"][-1], "stage3", final["stage3"][-1])


# ------------------------------------------------------------------ 6. errors
def test_bad_arguments_raise_and_the_next_call_works(loaded):  # noqa: F811
    le, canvas, sd = loaded["eng"], loaded["canvas"], loaded["sd"]
    base = le.backbone_train_taps(canvas)
    flat = lambda t: [t[0], *t[1], *t[2], *t[3]]  # noqa: E731
    w = {k: dev(sd[k]) for k in CONV}
    empty = ENG(small_cfg(24, 16, 2))
    with pytest.raises(RuntimeError):
        empty.backbone_train_taps(torch.zeros((1, 64, 24, 16), device="cuda"))  # no weights committed
    with pytest.raises(RuntimeError):
        empty.update_rpn_weights({k: torch.zeros(tuple(v.shape), device="cuda") for k, v in w.items()})
    with pytest.raises(ValueError):
        le.backbone_train_taps(canvas[:, :-1])
    with pytest.raises(TypeError):
        le.backbone_train_taps(canvas.cpu())
    try:
        le.set_precision("fp16")
        with pytest.raises(RuntimeError, match="fp32"):
            le.backbone_train_taps(canvas)
        with pytest.raises(RuntimeError, match="fp32"):
            le.update_rpn_weights(w)
    finally:
        le.set_precision("fp32")
    assert all(torch.equal(a, b) for a, b in zip(flat(le.backbone_train_taps(canvas)), flat(base)))
    with pytest.raises(ValueError):
        le.update_rpn_weights({**w, CONV[1]: w[CONV[1]][:-1]})
    with pytest.raises(ValueError):
        le.update_rpn_weights({**w, CONV[4]: w[CONV[5]]})  # a unit's shape where the strided convolution's belongs
    with pytest.raises(TypeError):
        le.update_rpn_weights({**w, CONV[7]: w[CONV[7]].cpu()})
    with pytest.raises(KeyError):
        le.update_rpn_weights({k: w[k] for k in CONV[:-1]})
    import ctypes
    ptrs = (ctypes.c_void_p * 16)(*([w[k].data_ptr() for k in CONV[:-1]] + [None]))
    assert le.lib.pp_update_rpn_weights(le.ctx, ptrs, None) != 0 and b"null" in le.lib.pp_last_error(le.ctx)
    # the narrower entry points keep refusing the other levels
    p5 = (ctypes.c_void_p * 5)(*[w[k].data_ptr() for k in CONV[5:10]])
    assert le.lib.pp_update_block_weights(le.ctx, 1, p5, 5, None) != 0 and b"block 3 only" in le.lib.pp_last_error(le.ctx)
    for level in (0, 1):
        with pytest.raises(RuntimeError, match="level 2 only"):
            le.update_down_weight(level, w[ENG.DOWN_KEYS[level]])
    le.update_rpn_weights(w)
    assert all(torch.equal(a, b) for a, b in zip(flat(le.backbone_train_taps(canvas)), flat(base)))
    assert torch.equal(le.backbone(canvas), base[0])  # the hooks are inert again
    # the autograd surface in a 16-bit mode, and the BatchNorm network
    net, _ = small_net()
    net.train(scope="rpn")
    cv = torch.zeros((1, 64, GX, GY), dtype=torch.float32, device="cuda")
    good = net.rpn_train(cv)
    net.half()
    with pytest.raises(RuntimeError, match="fp32"):
        net.rpn_train(cv)
    net.float()
    again = net.rpn_train(cv)
    assert again.requires_grad and torch.equal(again.detach(), good.detach())
    with pytest.raises(ValueError):
        net.rpn_train(cv[:, :, :-1])
    with pytest.raises(ValueError):
        net.train(scope="backbone")
    export = load_pkg("networks.pointpillars8_export")
    cfg = small_cfg(16, 16, 2)
    load_pkg("framework.voxel_generator").VoxelGenerator(cfg)
    with pytest.raises(RuntimeError, match="InstanceNorm"):
        export.PointPillars(cfg).train(scope="rpn")
