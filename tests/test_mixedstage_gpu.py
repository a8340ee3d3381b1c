"""GPU: the mixed-precision strided-stage and upsampler backwards (pp_down_backward_mp, csrc/down_train16.hip; pp_neck_backward_mp,
csrc/neck_train16.hip) through the engine wrappers and through the autograd surface PointPillars.train(scope=..., grad_precision=...,
grad_stages="rpn").

Bars.  Mode 0 is asserted equal, bit for bit, to the fp32 entries.  Modes 1 and 2 are held to the element-wise a-priori bounds of
tests/mixedstage_ref.py (derived there, cleared on the CPU by tests/test_mixedstage_cpu.py for every input set used here); every
largest fraction of a bound is printed.  Equality is asserted between identical calls, with and without dx, for a frame's dx
whatever batch it rides in, and between the autograd surface and the calls it makes.

Largest fractions of the bounds measured on an MI355X (the bound is 1): see DESIGN.md section 4, "Strided stages and upsamplers"."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import load_pkg
import mixedstage_ref as M
from train_common import dev, small_cfg, small_net, two_frames

pytestmark = pytest.mark.gpu
MODES = ("bf16x3", "bf16")
_ENGINES = {}


def engine(gx=24, gy=16, max_batch=3):
    """An engine without weights (both backwards are stateless), one per geometry for the whole module."""
    key = (gx, gy, max_batch)
    if key not in _ENGINES:
        load_pkg().install()
        _ENGINES[key] = load_pkg("engine").Engine(small_cfg(gx, gy, max_batch))
    return _ENGINES[key]


@functools.lru_cache(maxsize=None)
def down_set(shape):
    """The case, its tensors on the device and the mode-independent terms of its bounds: computed once, shared by both modes."""
    case = M.down_case(*shape)
    return case, [dev(t) for t in case], M.down_terms(*case)


@functools.lru_cache(maxsize=None)
def neck_set(shape):
    xs, ws, y, dy = M.neck_case(*shape)
    cases = [(xs[b], ws[b], y[:, M.branch_slice(b)], dy[:, M.branch_slice(b)]) for b in range(3)]
    return cases, ([dev(t) for t in xs], [dev(t) for t in ws], dev(y), dev(dy)), [M.neck_terms(*c) for c in cases]


def check(got, want, bound, what):
    frac, worst = M.worst(got.cpu().numpy(), want, bound)
    print(f"{what}: largest fraction of the a-priori bound {frac:.3f} (largest deviation {worst:.3e})")
    assert frac <= 1.0, (what, frac)
    return frac


def nan_like(shape):
    return torch.full(shape, float("nan"), device="cuda")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------ 1. mode 0 is the old call
def test_down_mode0_is_pp_down_backward():
    eng = engine()
    shape = M.DOWN_SHAPES[1]
    _, (xd, wd, zd, dyd), _ = down_set(shape)
    old = eng.down_backward(xd, wd, zd, dyd)
    new = eng.down_backward(xd, wd, zd, dyd, grad_precision="fp32")
    dw, dx = nan_like(tuple(wd.shape)), nan_like(tuple(xd.shape))
    assert eng.lib.pp_down_backward(eng.ctx, *shape[:4], ptr(xd), ptr(wd), ptr(zd), ptr(dyd), shape[4], ptr(dw), ptr(dx), None) == 0
    torch.cuda.synchronize()
    for a, b, c in zip(old, new, (dw, dx)):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert eng.down_backward_path("fp32", *shape[:4]) == "fp32"


def test_neck_mode0_is_pp_neck_backward():
    H, W, nb = M.NECK_MAPS[0]
    eng = engine(2 * H, 2 * W)
    _, (xs, ws, yd, dyd), _ = neck_set(M.NECK_MAPS[0])
    for b in range(3):
        old = eng.neck_backward(b, xs[b], ws[b], yd, dyd)
        new = eng.neck_backward(b, xs[b], ws[b], yd, dyd, grad_precision="fp32")
        dw, dx = nan_like(tuple(ws[b].shape)), nan_like(tuple(xs[b].shape))
        assert eng.lib.pp_neck_backward(eng.ctx, b, ptr(xs[b]), ptr(ws[b]), ptr(yd), ptr(dyd), nb, ptr(dw), ptr(dx), None) == 0
        torch.cuda.synchronize()
        for a, c, d in zip(old, new, (dw, dx)):
            assert torch.equal(a, c) and torch.equal(a, d)
        assert eng.neck_backward_path("fp32", b) == "fp32"


# ------------------------------------------------------------------ 2. shapes: tile edges, parities, halos, K ranges, plane segments
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", M.DOWN_SHAPES)
def test_down_shapes(shape, mode):
    eng = engine()
    case, (xd, wd, zd, dyd), t = down_set(shape)
    assert not t["ties"].any()
    assert eng.down_backward_path(mode, *shape[:4]) == mode
    dw, dx = eng.down_backward(xd, wd, zd, dyd, grad_precision=mode)
    rw, rx, bw, bx, _ = M.down_grad_bounds_mixed(*case, mode, terms=t)
    check(dw, rw, bw, f"down {shape} {mode} dw")
    check(dx, rx, bx, f"down {shape} {mode} dx")
    dw2, dx2 = eng.down_backward(xd, wd, zd, dyd, grad_precision=mode)
    dw3, none = eng.down_backward(xd, wd, zd, dyd, need_dx=False, grad_precision=mode)
    assert none is None and torch.equal(dw, dw2) and torch.equal(dx, dx2) and torch.equal(dw, dw3)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", M.NECK_MAPS)
def test_neck_shapes(shape, mode):
    H, W, nb = shape
    eng = engine(2 * H, 2 * W)
    cases, (xs, ws, yd, dyd), terms = neck_set(shape)
    for b in range(3):
        assert eng.neck_backward_path(mode, b) == mode
        dw, dx = eng.neck_backward(b, xs[b], ws[b], yd, dyd, grad_precision=mode)
        rw, rx, bw, bx = M.neck_grad_bounds_mixed(*cases[b], mode, terms=terms[b])
        check(dw, rw, bw, f"neck {shape} branch {b} {mode} dw")
        check(dx, rx, bx, f"neck {shape} branch {b} {mode} dx")
        dw2, dx2 = eng.neck_backward(b, xs[b], ws[b], yd, dyd, grad_precision=mode)
        dw3, none = eng.neck_backward(b, xs[b], ws[b], yd, dyd, need_dx=False, grad_precision=mode)
        assert none is None and torch.equal(dw, dw2) and torch.equal(dx, dx2) and torch.equal(dw, dw3)


# ------------------------------------------------------------------ 3. frames
@pytest.mark.parametrize("mode", MODES)
def test_down_frames(mode):
    eng = engine()
    shape = M.DOWN_SHAPES[1]  # two frames
    case, (xd, wd, zd, dyd), _ = down_set(shape)
    dw, dx = eng.down_backward(xd, wd, zd, dyd, grad_precision=mode)
    total, bound = 0.0, 0.0
    for f in range(2):
        s = slice(f, f + 1)
        dwf, dxf = eng.down_backward(xd[s].contiguous(), wd, zd[s].contiguous(), dyd[s].contiguous(), grad_precision=mode)
        assert torch.equal(dxf[0], dx[f]), f  # a frame's dx does not depend on the batch it rides in
        rw, _, bw, _, _ = M.down_grad_bounds_mixed(case[0][s], case[1], case[2][s], case[3][s], mode)
        check(dwf, rw, bw, f"down frame {f} {mode} dw")
        total, bound = total + dwf.cpu().numpy().astype(np.float64), bound + bw
    # the batch's dw against the sum of the frames' dw: each within its bound of the exact one, plus the batch's own summation
    rw, _, bw, _, _ = M.down_grad_bounds_mixed(*case, mode)
    check(dw, total, bound + bw, f"down batch {mode} dw against the frames'")


@pytest.mark.parametrize("mode", MODES)
def test_neck_frames(mode):
    H, W, _ = M.NECK_MAPS[2]  # two frames
    eng = engine(2 * H, 2 * W)
    cases, (xs, ws, yd, dyd), terms = neck_set(M.NECK_MAPS[2])
    for b in range(3):
        dw, dx = eng.neck_backward(b, xs[b], ws[b], yd, dyd, grad_precision=mode)
        total, bound = 0.0, 0.0
        for f in range(2):
            s = slice(f, f + 1)
            dwf, dxf = eng.neck_backward(b, xs[b][s].contiguous(), ws[b], yd[s].contiguous(), dyd[s].contiguous(), grad_precision=mode)
            assert torch.equal(dxf[0], dx[f]), (b, f)
            rw, _, bw, _ = M.neck_grad_bounds_mixed(cases[b][0][s], cases[b][1], cases[b][2][s], cases[b][3][s], mode)
            check(dwf, rw, bw, f"neck branch {b} frame {f} {mode} dw")
            total, bound = total + dwf.cpu().numpy().astype(np.float64), bound + bw
        _, _, bw, _ = M.neck_grad_bounds_mixed(*cases[b], mode, terms=terms[b])
        check(dw, total, bound + bw, f"neck branch {b} batch {mode} dw against the frames'")


# ------------------------------------------------------------------ 4. the modes are told apart
def told_apart(dws, rw, bw_plain, what):
    d16 = np.abs(dws["bf16"].cpu().numpy().astype(np.float64) - rw)
    d3 = np.abs(dws["bf16x3"].cpu().numpy().astype(np.float64) - rw)
    frac, ratio = float((d16 / bw_plain).max()), float(d3.max() / d16.max())
    print(f"{what}: bf16 dw at {frac:.1f} x the fp32 bound, bf16x3 / bf16 deviation {ratio:.4f}")
    assert frac > 1.0, (what, frac)       # the 16-bit kernel ran: fp32 arithmetic cannot leave its own bound
    assert ratio < 1.0 / 16, (what, ratio)  # and the split form is not the plain form


def test_down_modes_are_told_apart():
    eng = engine()
    case, args, t = down_set(M.DOWN_APART)
    told_apart({m: eng.down_backward(*args, grad_precision=m)[0] for m in MODES}, t["dw"], t["bw"], "down")


def test_neck_modes_are_told_apart():
    H, W, _ = M.NECK_APART
    eng = engine(2 * H, 2 * W)
    b = M.NECK_APART_BRANCH
    _, (xs, ws, yd, dyd), terms = neck_set(M.NECK_APART)
    told_apart({m: eng.neck_backward(b, xs[b], ws[b], yd, dyd, grad_precision=m)[0] for m in MODES}, terms[b]["dw"], terms[b]["bw"], "neck")


# ------------------------------------------------------------------ 5. path query
def test_path_query():
    eng = engine()
    for mode in ("fp32",) + MODES:
        for shape in ((64, 64, 800, 800), (64, 128, 400, 400), (128, 256, 200, 200)):  # the network's stages on a 400 x 400 map
            assert eng.down_backward_path(mode, *shape) == mode, (mode, shape)
    big = engine(800, 800, 1)  # level-0 map 400 x 400
    assert (big.H, big.W) == (400, 400)
    for mode in ("fp32",) + MODES:
        for b in range(3):
            assert big.neck_backward_path(mode, b) == mode, (mode, b)
    # the 16-bit kernels read the fp32 planes, so no shape falls back: a frame past the fp32 planes' 256 MB budget
    # ((4 x 64 + 64) planes of 502 x 502 elements and their guards: 323 MB) is refused by the query as by the entry
    for mode in MODES:
        with pytest.raises(RuntimeError, match="map too large"):
            eng.down_backward_path(mode, 64, 64, 1000, 1000)
    for bad in ("fp16", 2, None):
        with pytest.raises(ValueError):
            eng.down_backward_path(bad, 64, 64, 40, 40)
        with pytest.raises(ValueError):
            eng.neck_backward_path(bad, 0)
    with pytest.raises(RuntimeError, match="cin, cout"):
        eng.down_backward_path("bf16", 128, 128, 40, 40)
    with pytest.raises(RuntimeError, match="cin, cout"):
        eng.down_backward_path("bf16", 64, 256, 40, 40)
    with pytest.raises(ValueError):
        eng.neck_backward_path("bf16", 3)
    assert eng.lib.pp_neck_backward_path(eng.ctx, 2, 3) < 0 and b"branch" in eng.lib.pp_last_error(eng.ctx)
    assert eng.lib.pp_down_backward_path(eng.ctx, 3, 64, 64, 40, 40) < 0 and b"mode" in eng.lib.pp_last_error(eng.ctx)
    assert eng.lib.pp_neck_backward_path(eng.ctx, -1, 0) < 0 and b"mode" in eng.lib.pp_last_error(eng.ctx)


# ------------------------------------------------------------------ 6. autograd surface
def test_autograd_surface(monkeypatch):
    load_pkg().install()
    net, _ = small_net()
    eng = net._eng
    shared = load_pkg("networks.pointpillars8_shared")
    example = two_frames(eng)
    with torch.no_grad():
        plain = net(example)
    rng = np.random.default_rng(8)
    up = {k: dev(rng.standard_normal(tuple(v.shape)).astype(np.float32) * np.float32(1e-2)) for k, v in plain.items()}
    downs, necks = [], []
    inner_down, inner_neck = eng.down_backward, eng.neck_backward

    def rec_down(x, w, z, dy, need_dx=True, **kw):
        out = inner_down(x, w, z, dy, need_dx=need_dx, **kw)
        downs.append((w, (x, z, dy), kw, out[0]))
        return out

    def rec_neck(branch, x, w, y, dy, need_dx=True, **kw):
        out = inner_neck(branch, x, w, y, dy, need_dx=need_dx, **kw)
        necks.append((w, (branch, x, y, dy), kw, out[0]))
        return out

    monkeypatch.setattr(eng, "down_backward", rec_down)
    monkeypatch.setattr(eng, "neck_backward", rec_neck)

    def grads_of(**kw):
        net.train(scope="rpn", **kw)
        preds = net(example)
        for k in plain:
            assert torch.equal(preds[k].detach(), plain[k]), k  # the training forward stays fp32: the inference bits
        net.zero_grad()
        del downs[:], necks[:]
        sum((preds[k] * up[k]).sum() for k in preds).backward()
        return {k: p.grad.clone() for k, p in net.named_parameters()}, list(downs), list(necks)

    fp32, d0, n0 = grads_of()
    assert net.grad_stages == "units" and len(d0) == 3 and len(n0) == 3 and not any(c[2] for c in d0 + n0)  # the old signatures
    for kw in (dict(grad_stages="rpn"), dict(grad_precision="fp32", grad_stages="rpn")):
        same, d1, n1 = grads_of(**kw)
        assert not any(c[2] for c in d1 + n1)  # fp32: the keyword is not passed at all
        for k in fp32:
            assert torch.equal(fp32[k], same[k]), k
    for mode in MODES:
        unnamed, _, _ = grads_of(grad_precision=mode)
        units, du, nu = grads_of(grad_precision=mode, grad_stages="units")
        assert not any(c[2] for c in du + nu)
        for k in unnamed:
            assert torch.equal(unnamed[k], units[k]), k  # "units" is the behaviour of a call that never names the keyword
        got, ds, ns = grads_of(grad_precision=mode, grad_stages="rpn")
        assert (net.grad_precision, net.grad_stages) == (mode, "rpn")
        assert len(ds) == 3 and len(ns) == 3 and all(c[2] == {"grad_precision": mode} for c in ds + ns)
        for k in shared.HEAD_KEYS:  # what runs in front of the first stage backward did not change
            assert torch.equal(got[k], fp32[k]), k
        params = dict(net.named_parameters())
        by_weight = {c[0].data_ptr(): c for c in ds + ns}
        for k in eng.DOWN_KEYS:
            w, (x, z, dy), _, dw = by_weight[params[k].data_ptr()]
            assert torch.equal(dw, got[k]) and not torch.equal(got[k], units[k]), k
            rw, _, bw, _, ties = M.down_grad_bounds_mixed(*(t.detach().cpu().numpy() for t in (x, params[k], z, dy)), mode)
            assert ties.sum() <= 1e-3 * ties.size, k
            check(dw, rw, bw, f"{mode} autograd dw {k}")
        for k in eng.NECK_KEYS:
            w, (b, x, y, dy), _, dw = by_weight[params[k].data_ptr()]
            assert torch.equal(dw, got[k]) and not torch.equal(got[k], units[k]), k
            sl = M.branch_slice(b)
            rw, _, bw, _ = M.neck_grad_bounds_mixed(*(t.detach().cpu().numpy() for t in (x, params[k], y[:, sl], dy[:, sl])), mode)
            check(dw, rw, bw, f"{mode} autograd dw {k}")
    with pytest.raises(ValueError):
        net.train(scope="rpn", grad_stages="all")
    net.train(scope="rpn", grad_precision="bf16", grad_stages="rpn")
    net.eval()
    assert (net.grad_precision, net.grad_stages) == ("fp32", "units")
    again, _, _ = grads_of()
    for k in fp32:
        assert torch.equal(fp32[k], again[k]), k


# ------------------------------------------------------------------ 7. it trains
@pytest.mark.parametrize("mode", MODES)
def test_it_trains(mode):
    """The twenty Adam steps of test_mixedtrain_gpu.test_it_trains (lr 1e-3, clip_grad_norm_ 10, a fixed batch of two frames, scope
    "rpn") with the strided stages and upsamplers in the mode as well.  A sanity condition, not a measurement."""
    load_pkg().install()
    LossGenerator = load_pkg("framework.loss_generator").LossGenerator
    net, cfg = small_net()
    eng = net._eng
    example = two_frames(eng)
    rng = np.random.default_rng(21)
    u = rng.random((2, eng.A))
    labels = np.where(u < 1 / 7, 1, np.where(u < 0.75, 0, -1)).astype(np.int32)
    ex = {"labels": labels, "bbox_targets": (rng.standard_normal((2, eng.A, 7)) * 0.4).astype(np.float32) * (labels > 0)[..., None],
          "dir_targets": (rng.random((2, eng.A)) < 0.5).astype(np.int32)}
    lg = LossGenerator(cfg)
    net.train(scope="rpn", grad_precision=mode, grad_stages="rpn")
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    losses = []
    for _ in range(20):
        loss = lg.generate(net(example), ex)["loss"]
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(net.parameters()), 10.0)
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(lg.generate(net(example), ex)["loss"]))
    print(mode, " ".join(f"{v:.6f}" for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < 0.5 * losses[0], (mode, losses)


# ------------------------------------------------------------------ 8. errors
def test_bad_arguments_return_an_error_and_the_next_call_works():
    eng = engine()
    shape = M.DOWN_SHAPES[0]
    _, (xd, wd, zd, dyd), _ = down_set(shape)
    good = eng.down_backward(xd, wd, zd, dyd, grad_precision="bf16")
    spare = [torch.empty_like(good[0]), torch.empty_like(good[1])]  # never written: every call below is refused before it launches
    out = [ptr(t) for t in spare]
    p = [ptr(xd), ptr(wd), ptr(zd), ptr(dyd)]
    lib, nb = eng.lib, shape[4]
    odd = ctypes.c_void_p(wd.data_ptr() + 4)
    for mode, dims, args, n in ((3, shape[:4], p, nb), (-1, shape[:4], p, nb), (2, shape[:4], [p[0], odd, p[2], p[3]], nb),
                                (2, shape[:4], [None] + p[1:], nb), (1, shape[:4], p, 0), (1, shape[:4], p, eng.max_batch + 1),
                                (2, (96, 64) + shape[2:4], p, nb)):
        assert lib.pp_down_backward_mp(eng.ctx, mode, *dims, *args, n, *out, None) != 0, (mode, dims, n)
        assert b"pp_down_backward_mp" in lib.pp_last_error(eng.ctx)
    for bad in ("fp16", 2):
        with pytest.raises(ValueError):
            eng.down_backward(xd, wd, zd, dyd, grad_precision=bad)
    again = eng.down_backward(xd, wd, zd, dyd, grad_precision="bf16")
    assert torch.equal(good[0], again[0]) and torch.equal(good[1], again[1])

    H, W, nb = M.NECK_MAPS[1]
    eng = engine(2 * H, 2 * W)
    _, (xs, ws, yd, dyd), _ = neck_set(M.NECK_MAPS[1])
    good = eng.neck_backward(1, xs[1], ws[1], yd, dyd, grad_precision="bf16x3")
    spare = [torch.empty_like(good[0]), torch.empty_like(good[1])]  # never written: every call below is refused before it launches
    out = [ptr(t) for t in spare]
    p = [ptr(xs[1]), ptr(ws[1]), ptr(yd), ptr(dyd)]
    odd = ctypes.c_void_p(ws[1].data_ptr() + 4)
    for mode, b, args, n in ((3, 1, p, nb), (1, 3, p, nb), (1, 1, [p[0], odd, p[2], p[3]], nb), (2, 1, p[:2] + [None, p[3]], nb), (2, 1, p, 0),
                             (2, 1, p, eng.max_batch + 1)):
        assert eng.lib.pp_neck_backward_mp(eng.ctx, mode, b, *args, n, *out, None) != 0, (mode, b, n)
        assert b"pp_neck_backward_mp" in eng.lib.pp_last_error(eng.ctx)
    for bad in ("fp16", 1):
        with pytest.raises(ValueError):
            eng.neck_backward(1, xs[1], ws[1], yd, dyd, grad_precision=bad)
    again = eng.neck_backward(1, xs[1], ws[1], yd, dyd, grad_precision="bf16x3")
    assert torch.equal(good[0], again[0]) and torch.equal(good[1], again[1])
