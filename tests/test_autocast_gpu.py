"""GPU: the training forward on 16-bit MFMA operands, train(forward_precision="bf16x3" | "bf16" | "fp16").

What is new underneath is the in-place writer of the 16-bit weight images (csrc/image16.hip) behind pp_update_{rpn,neck,head}_weights_mp,
and pp_backbone_train_taps_mp, the tapped pass on a plan committed in a 16-bit mode.  Everything is held against what the project
already trusts: the images against those a fresh engine packs from the same values in that mode, bit for bit; the training forward
against the eval-mode forward of a fresh network in that mode, bit for bit; the taps against their own norm at the fp32 taps test's bar
and against the fp32 engine's taps at the project's per-mode deviation bars (PRECISION_BARS); the gradients against the fp32 run's.
Grids: 64 x 96 cells, where every layer takes a 16-bit tiling; 32 x 24 cells, whose level-2 map is 4 x 3, so that layers may stay on
fp32 tilings in a 16-bit plan (whatever mix layer_tilings() reports is handled, and printed); and the 48 x 32 cells of train_common
with its two frames for everything that runs a network.  Engines that are compared are
created in one process, so the tuner's table gives them the same tilings; that is asserted."""
import functools
import re

import numpy as np
import pytest
import torch

from conftest import load_pkg
import arena as A
import rpntrain_ref as R
from test_gpu_frames import PRECISION_BARS
from train_common import GX, GY, canvases_of, dev, seeded_sd, small_cfg, two_frames

pytestmark = pytest.mark.gpu
ENG = load_pkg("engine").Engine
CONV, NECK, HEAD = ENG.RPN_CONV_KEYS, ENG.NECK_KEYS, ENG.HEAD_KEYS
MODES = ("bf16x3", "bf16", "fp16")
GRIDS = {"all16": (64, 96), "odd": (32, 24), "small": (GX, GY)}
BAR = 2e-4  # the fp32 taps test's bar (test_rpntrain_gpu.py)
# 4 x the largest max-norm relative deviation of a gradient tensor from the fp32 run's, measured on the MI355X per mode (the values
# are in DESIGN.md section 4), rounded up to one digit.  The operand rounding is deterministic; what varies between plans is fp32
# summation order, for which 4 x is ample.
GRAD_BARS = {"bf16x3": 2e-4, "bf16": 3.0, "fp16": 2.0}  # measured 3.6e-5, 0.60, 0.27


def shared():
    return load_pkg("networks.pointpillars8_shared")


def make_net(grid, sd=None, precision=None):
    load_pkg().install()
    cfg = small_cfg(*GRIDS[grid], 4)
    load_pkg("framework.voxel_generator").VoxelGenerator(cfg)
    net = shared().PointPillars(cfg)
    net.profile_stages = False
    if precision:
        net.precision(precision)
    net.load_state_dict(sd if sd is not None else load_pkg("synth").seeded_state_dict(0))
    return net, cfg


def canvas_of(grid, seed=3, n=300):
    gx, gy = GRIDS[grid]
    rng = np.random.default_rng(seed)
    canvas = np.zeros((1, 64, gx, gy), np.float32)
    cells = rng.choice(gx * gy, n, replace=False)
    canvas[0, :, cells // gy, cells % gy] = np.maximum(rng.standard_normal((n, 64)), 0).astype(np.float32)
    return dev(canvas)


def is16(t):
    """Does a layer of layer_tilings() run a 16-bit tiling?  conv16's and gemm1x1's 16-bit tilings carry their operand mode, p1 | p2 | p3,
    in their names; the fp32 tilings have no such token."""
    return re.search(r" p[123]( |$)", t["tiling"]) is not None


def all_images(eng):
    return [eng.weight_image(i).clone() for i in range(20)]


def upload(eng, vals, mode):
    eng.update_rpn_weights({k: dev(vals[k]) for k in CONV}, forward_precision=mode)
    eng.update_neck_weights({k: dev(vals[k]) for k in NECK}, forward_precision=mode)
    eng.update_head_weights({k: dev(vals[k]) for k in HEAD}, forward_precision=mode)


def perturbed(sd, rng):
    new = dict(sd)
    for k in CONV + NECK + HEAD:
        new[k] = sd[k] + rng.standard_normal(sd[k].shape).astype(np.float32) * np.float32(0.02)
    return new


# ------------------------------------------------------------------ 1. the images, bit for bit
@pytest.mark.parametrize("grid", ["all16", "odd"])
@pytest.mark.parametrize("mode", MODES)
def test_images_bit_for_bit(mode, grid):
    sd = seeded_sd()
    net, cfg = make_net(grid)
    eng = net._eng
    assert not any(is16(t) for t in eng.layer_tilings())
    net.train(scope="rpn", forward_precision=mode)
    assert net.forward_precision == mode and eng.effective_precision() == mode
    til = eng.layer_tilings()
    assert len(til) == 20
    kept = [i for i, t in enumerate(til) if not is16(t)]
    print(f"{mode} {grid}: layers on an fp32 tiling in the 16-bit plan: {kept} {[til[i]['tiling'] for i in kept]}")
    if grid == "all16":
        assert kept == [], "64 x 96 cells: every layer takes a 16-bit tiling"
    rng = np.random.default_rng(5)
    new = perturbed(sd, rng)
    want = {}
    for which, vals in (("old", sd), ("new", new)):
        fresh = ENG(small_cfg(*GRIDS[grid], 4), precision=mode)
        fresh.load_state_dict(vals)
        assert fresh.layer_tilings() == til
        want[which] = all_images(fresh)
    assert not any(torch.equal(a, b) for a, b in zip(want["old"], want["new"]))
    if mode == "bf16x3" and grid == "all16":  # the lo halves are there and are not empty: a split image is twice a plain one's size
        plain = ENG(small_cfg(*GRIDS[grid], 4), precision="bf16")
        plain.load_state_dict(sd)
        sizes = [(a.numel(), b.numel()) for a, b, t in zip(want["old"], all_images(plain), til) if t["kind"] == 0]
        assert all(a == 2 * b for a, b in sizes), sizes
    for which, vals in (("old", sd), ("new", new), ("old", sd)):  # the committed values, perturbed ones, and back
        upload(eng, vals, mode)
        for i, (a, b) in enumerate(zip(all_images(eng), want[which])):
            assert a.shape == b.shape and torch.equal(a, b), (which, i, til[i]["tiling"])


# ------------------------------------------------------------------ 2. the forward, bit for bit
@pytest.mark.parametrize("mode", MODES)
def test_forward_bit_for_bit(mode):
    net, cfg = make_net("small")
    eng = net._eng
    example = two_frames(eng)
    canvases = torch.cat(canvases_of(eng, example))
    other, _ = make_net("small", precision=mode)
    net.train(scope="rpn", forward_precision=mode)
    assert other._eng.layer_tilings() == eng.layer_tilings() and other._eng.effective_precision() == mode

    def same():
        y = net.rpn_train(canvases)
        assert y.requires_grad and torch.equal(y.detach(), torch.cat([other.rpn(c) for c in canvases]))
        got, want = net(example), other(example)
        assert all(got[k].requires_grad and torch.equal(got[k].detach(), want[k]) for k in want)
        return got

    same()
    LossGenerator = load_pkg("framework.loss_generator").LossGenerator
    lg, ex = LossGenerator(cfg), targets(eng)
    opt = load_pkg("framework.optim").Adam(net.parameters(), lr=1e-3)
    for _ in range(3):
        loss = lg.generate(net(example), ex)["loss"]
        opt.zero_grad()
        loss.backward()
        opt.step()
    sd = net.state_dict()
    start = seeded_sd()
    for k in (CONV[0], CONV[7], NECK[1], HEAD[0]):
        assert np.abs(sd[k] - start[k].reshape(sd[k].shape)).max() > 1e-4, k
    other.load_state_dict(sd)
    assert other._eng.layer_tilings() == eng.layer_tilings()
    same()  # upload and forward together
    for i, (a, b) in enumerate(zip(all_images(eng), all_images(other._eng))):
        assert torch.equal(a, b), i


def targets(eng, seed=21):
    rng = np.random.default_rng(seed)
    u = rng.random((2, eng.A))
    labels = np.where(u < 1 / 7, 1, np.where(u < 0.75, 0, -1)).astype(np.int32)
    return {"labels": labels, "bbox_targets": (rng.standard_normal((2, eng.A, 7)) * 0.4).astype(np.float32) * (labels > 0)[..., None],
            "dir_targets": (rng.random((2, eng.A)) < 0.5).astype(np.int32)}


# ------------------------------------------------------------------ 3. the taps
@functools.lru_cache(maxsize=None)
def fp32_taps(grid):
    load_pkg().install()
    eng = ENG(small_cfg(*GRIDS[grid], 2))
    eng.load_state_dict(seeded_sd())
    return eng.backbone_train_taps(canvas_of(grid))


@pytest.mark.parametrize("grid", ["all16", "odd"])
@pytest.mark.parametrize("mode", MODES)
def test_taps(mode, grid):
    ref = fp32_taps(grid)
    canvas = canvas_of(grid)
    eng = ENG(small_cfg(*GRIDS[grid], 2), precision=mode)
    eng.load_state_dict(seeded_sd())
    plain = eng.backbone(canvas).clone()
    y, xs, units, zs = eng.backbone_train_taps(canvas, forward_precision=mode)
    assert torch.equal(y, plain)
    bar = PRECISION_BARS[mode][0]
    flat = lambda t: {"y": t[0], **{f"x{b}": t[1][b] for b in range(3)}, **{f"units{b}[{k}]": t[2][b][k] for b in range(3) for k in range(ENG.RPN_UNITS[b])},  # noqa: E731
                      **{f"z{b}": t[3][b] for b in range(3)}}
    got, want = flat((y, xs, units, zs)), flat(ref)
    for name in want:
        scale = float(want[name].abs().max())
        err = float((got[name] - want[name]).abs().max())
        print(f"{mode} {grid} {name}: deviation from the fp32 engine's tap {err:.3e} = {err / scale:.2e} of max |tap| {scale:.3f} (bar {bar:g})")
        assert got[name].shape == want[name].shape and scale > 0 and err <= bar * scale, name
    for b in range(3):
        z = zs[b].cpu().numpy()
        u0 = units[b][0].cpu().numpy().astype(np.float64)
        err = np.abs(np.maximum(R.B.norm(z)[0], 0.0)[0] - u0).max()
        print(f"{mode} {grid} level {b}: units[0] against relu(norm(z)) {err:.3e}")
        assert err <= BAR and u0.min() >= 0 and u0.max() > 0, b
    assert torch.equal(eng.backbone(canvas), plain)  # the hooks are inert again
    again = eng.backbone_train_taps(canvas, forward_precision=mode)
    assert all(torch.equal(a, b) for a, b in zip(flat(again).values(), got.values()))


# ------------------------------------------------------------------ 4. gradients
def one_backward(mode, steps=0):
    """The fixture's loss.backward() under scope="rpn" -> {name: gradient}; with steps > 0 the losses of that many Adam steps behind it."""
    net, cfg = make_net("small")
    eng = net._eng
    example = two_frames(eng)
    lg, ex = load_pkg("framework.loss_generator").LossGenerator(cfg), targets(eng)
    net.train(scope="rpn", **({} if mode == "fp32" else {"forward_precision": mode}))
    loss = lg.generate(net(example), ex)["loss"]
    net.zero_grad()
    loss.backward()
    grads = {k: p.grad.clone() for k, p in net.named_parameters()}
    losses = [float(loss.detach())]
    if steps:
        opt = load_pkg("framework.optim").Adam(net.parameters(), lr=1e-3)
        for i in range(steps):
            if i:
                loss = lg.generate(net(example), ex)["loss"]
                opt.zero_grad()
                loss.backward()
                losses.append(float(loss.detach()))
            torch.nn.utils.clip_grad_norm_(list(net.parameters()), 10.0)
            opt.step()
        with torch.no_grad():
            losses.append(float(lg.generate(net(example), ex)["loss"]))
    return grads, losses


@functools.lru_cache(maxsize=None)
def fp32_backward():
    return one_backward("fp32")[0]


@pytest.mark.parametrize("mode", MODES)
def test_gradients_and_descent(mode):
    """One backward against the fp32 run's gradients of the same fixture (the existing fp32 path is the reference), then twenty Adam
    steps (lr 1e-3, clip 10: test_rpntrain_gpu.test_trajectory's loop, whose fp32 run ends at 0.0976) on the fixed batch."""
    ref = fp32_backward()
    grads, losses = one_backward(mode, steps=20)
    assert set(grads) == set(ref) and len(grads) == 25
    worst = 0.0
    for k, g in grads.items():
        dev_ = float((g - ref[k]).abs().max()) / float(ref[k].abs().max())
        worst = max(worst, dev_)
        print(f"[autocast grad] {mode} {k}: max-norm relative deviation from the fp32 run's gradient {dev_:.3e}")
    print(f"[autocast grad] {mode}: largest {worst:.3e}, bar {GRAD_BARS[mode]}")
    print(f"[autocast descent] {mode}: " + " ".join(f"{v:.6f}" for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert GRAD_BARS[mode] is not None and worst <= GRAD_BARS[mode], (mode, worst)


# ------------------------------------------------------------------ 5. mode switches
def test_mode_switches():
    net, cfg = make_net("small")
    eng = net._eng
    example = two_frames(eng)
    single = {k: v for k, v in canvases_example(eng).items()}
    lg, ex = load_pkg("framework.loss_generator").LossGenerator(cfg), targets(eng)
    net.train(scope="rpn")
    opt = load_pkg("framework.optim").Adam(net.parameters(), lr=1e-3)
    for _ in range(2):
        loss = lg.generate(net(example), ex)["loss"]
        opt.zero_grad()
        loss.backward()
        opt.step()
    net.eval()
    sd = net.state_dict()
    net.half()  # the stepped groups go up in place into the fp16 images
    with torch.no_grad():
        got = net(single)
    other, _ = make_net("small", sd=sd, precision="fp16")
    assert other._eng.layer_tilings() == eng.layer_tilings() and eng.effective_precision() == "fp16"
    with torch.no_grad():
        want = other(single)
    assert all(torch.equal(got[k], want[k]) for k in want)
    for mode in ("bf16x3", "bf16"):
        net.precision(mode)
        other.precision(mode)
        with torch.no_grad():
            got, want = net(single), other(single)
        assert all(torch.equal(got[k], want[k]) for k in want), mode
    net.float()
    other, _ = make_net("small", sd=sd)
    with torch.no_grad():
        got, want = net(single), other(single)
    assert all(torch.equal(got[k], want[k]) for k in want)
    # the fused fp32 pass reads the sparse first convolution's image, and tile skipping is armed again where the map allows it
    rng = np.random.default_rng(9)
    pts = dev(rng.uniform([0, 0, -1.5, 0], [0.2 * GX, 0.2 * GY, 1.0, 1], (3000, 4)).astype(np.float32))
    da, db = eng.infer_frame(pts), other._eng.infer_frame(pts)
    assert int(eng.fetch(0, "active")[0]) > 0  # the sparse first convolution ran
    assert eng.tile_skip_active() == other._eng.tile_skip_active()
    assert torch.equal(eng.fetch(0, "rpn"), other._eng.fetch(0, "rpn")) and all(torch.equal(x, y) for x, y in zip(da, db))
    assert torch.equal(eng.weight_image(-1), other._eng.weight_image(-1))
    # a 16-bit training forward whose engine was switched away
    net.train(scope="rpn", forward_precision="fp16")
    assert net(example)["cls_preds"].requires_grad
    net.float()
    with pytest.raises(RuntimeError, match="fp16"):
        net(example)
    with pytest.raises(RuntimeError, match="fp16"):
        net.rpn_train(torch.cat(canvases_of(eng, example)))
    net.eval()
    assert net.forward_precision == "fp32"
    # fp16s has no in-place writer: stepped weights need a reload there
    net.train(scope="rpn")
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0)
    net.eval()
    net.precision("fp16s")
    if eng.effective_precision() == "fp16s":
        with pytest.raises(RuntimeError, match="load_state_dict"), torch.no_grad():
            net(single)
    net.float()


def canvases_example(eng):
    """A single frame as forward() takes it (coordinates [n,3])."""
    rng = np.random.default_rng(14)
    n = 220
    cells = rng.choice(GX * GY, n, replace=False)
    coors = np.stack([cells // GY, cells % GY, np.zeros(n, np.int64)], 1).astype(np.int32)
    return {"voxels": dev(rng.standard_normal((n, eng.T, eng.F)).astype(np.float32)), "coordinates": dev(coors),
            "num_points_per_voxel": dev(rng.integers(1, eng.T + 1, n).astype(np.int32))}


# ------------------------------------------------------------------ 6. the writer on arenas
@pytest.mark.parametrize("mode", MODES)
def test_writer_on_arenas(mode):
    """k_image16 through pp_debug_image16: the image starts as 0xA5 inside guard bands, the weight tensors sit in arenas of zeros
    and of NaNs.  No byte outside the image changes, no element keeps 0xA5 (padding is written as 0), the image has the same bits
    under every fill, and they are the committed image's."""
    load_pkg().install()
    sd = seeded_sd()
    eng = ENG(small_cfg(*GRIDS["all16"], 2), precision=mode)
    eng.load_state_dict(sd)
    til = eng.layer_tilings()
    picks = [0, 1, next(i for i, t in enumerate(til) if t["kind"] == 1 and t["up"] == 4), 19]  # a strided conv, a unit, an upsampler, the head
    for layer in picks:
        t = til[layer]
        keys = [k for k in HEAD if k.endswith("weight")] if t["kind"] == 2 else [(list(CONV) + list(NECK))[conv_or_neck(til, layer)]]
        want = eng.weight_image(layer)
        outs = []
        for fill, pre in (("zeros", "a5"), ("nan", "5a")):  # two pre-fills: an element the kernel never stored differs between the runs
            ws = [A.place(dev(sd[k]).reshape(-1), fill=fill) for k in keys]
            out = A.place_out((want.numel() // 2,), torch.int16, fill=pre)
            eng.debug_image16(layer, [w.t for w in ws], out=out.buf[out.lo:out.hi])
            torch.cuda.synchronize()
            assert all(A.untouched(w) for w in ws) and A.untouched(out), (layer, fill)
            # no element keeps 0xA5: the pattern is a value a weight can round to (fp16 -0.0221), so it occurs as often as in the committed image
            assert out.stale() == int((want.view(torch.int16) == -23131).sum()), (layer, fill, "an element kept 0xA5")
            outs.append(out.t.clone())
        assert torch.equal(outs[0], outs[1]), layer
        assert torch.equal(outs[0].view(torch.uint8), want), (layer, t["tiling"])
        if t["kind"] == 2:
            assert int((outs[0] == 0).sum()) > 0  # the head's rows 90 .. 95 are padding


def conv_or_neck(til, layer):
    """layer of layer_tilings() -> its index in CONV + NECK."""
    kind = til[layer]["kind"]
    ordinal = sum(1 for t in til[:layer] if t["kind"] == kind)
    return ordinal if kind == 0 else 16 + ordinal


# ------------------------------------------------------------------ 7. refusals
def test_refusals():
    load_pkg().install()
    sd = seeded_sd()
    eng = ENG(small_cfg(GX, GY, 2), precision="bf16")
    eng.load_state_dict(sd)
    canvas = canvas_of("small")
    w = {k: dev(sd[k]) for k in CONV + NECK + HEAD}
    calls = (lambda m: eng.backbone_train_taps(canvas, forward_precision=m), lambda m: eng.update_rpn_weights(w, forward_precision=m),
             lambda m: eng.update_neck_weights(w, forward_precision=m), lambda m: eng.update_head_weights(w, forward_precision=m))
    before = all_images(eng)
    for call in calls:
        for other in ("fp16", "bf16x3"):
            with pytest.raises(RuntimeError, match="bf16"):  # names both modes
                call(other)
        for bad in ("fp16s", "half", None):
            with pytest.raises(ValueError, match="forward_precision"):
                call(bad)
        with pytest.raises(RuntimeError, match="fp32"):  # the default keeps today's refusal
            call("fp32")
        call("bf16")
    assert all(torch.equal(a, b) for a, b in zip(all_images(eng), before))
    # the library's own guard, behind the engine's
    import ctypes
    ptrs = (ctypes.c_void_p * 16)(*[w[k].data_ptr() for k in CONV])
    for bad in (0, 1, 3, 4, 5):
        assert eng.lib.pp_update_rpn_weights_mp(eng.ctx, bad, ptrs, None) == 1, bad
    assert eng.lib.pp_update_rpn_weights_mp(eng.ctx, 2, ptrs, None) == 0
    eng.set_precision("fp16s")
    if eng.effective_precision() == "fp16s":
        for m in (3, 4):
            assert eng.lib.pp_update_rpn_weights_mp(eng.ctx, m, ptrs, None) == 1
    # module level
    net, _ = make_net("small")
    for bad in ("fp16s", "half"):
        with pytest.raises(ValueError, match="forward_precision"):
            net.train(scope="rpn", forward_precision=bad)
    assert net.train(scope="rpn", forward_precision="bf16").forward_precision == "bf16"
    assert net.eval().forward_precision == "fp32"
    export = load_pkg("networks.pointpillars8_export")
    cfg = small_cfg(16, 16, 2)
    load_pkg("framework.voxel_generator").VoxelGenerator(cfg)
    with pytest.raises(ValueError, match="forward_precision"):
        export.PointPillars(cfg).train(scope="rpn", bn_stats="frozen", forward_precision="fp16")
