"""GPU: mixed-precision training -- the Resnet unit backward with bf16x3 / bf16 operands (pp_unit_backward_mp, csrc/block_train16.hip)
through the engine wrappers and through the autograd surface PointPillars.train(scope=..., grad_precision=...).

Bars.  Everything numeric: the element-wise a-priori bounds of tests/mixedtrain_ref.grad_bounds_mixed (blocktrain_ref.grad_bounds with
the two product terms widened by the bf16 operand error and, for bf16x3, by its three MFMAs per product; derived there).  That the
16-bit kernels really ran is shown by pp_unit_backward_path, by plain bf16 leaving the fp32 bound, and by bf16x3 being at least 16
times closer to float64 than bf16.  Equality is asserted between fp32 mode and the old call, between identical calls, with and
without du, for the dskip add, for a frame's du whatever batch it rides in, and for every gradient whose backward did not change.
Random inputs go through blocktrain_ref.tie_free, so no ReLU argument lies within 1e-4 of zero (asserted).

Shares of the bounds measured on gfx950 (largest fraction over the seven shapes of test_shapes): bf16 dw 0.93 (the 3 x 2 map, 12 terms
per sum; 0.12 on the maps of a few hundred positions), du 0.07; bf16x3 dw 0.47 (same map; 0.015), du 0.006.  Through the autograd
surface, per unit: bf16 dw up to 0.81, bf16x3 up to 0.35.  bf16's dw leaves the fp32 bound by 26 x at its worst element, and its
largest deviation is 458 x that of bf16x3.  Final loss of test_it_trains: bf16x3 0.097373, bf16 0.097429, from 1.555734."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_pkg
import blocktrain_ref as R
import mixedtrain_ref as M
from train_common import check_bound, dev, small_cfg, small_net, two_frames

pytestmark = pytest.mark.gpu
MODES = ("bf16x3", "bf16")
SHAPES = [(64, 33, 17, 1), (128, 20, 18, 2), (256, 25, 9, 3), (256, 1, 7, 2), (256, 2, 20, 1), (256, 3, 2, 2), (64, 130, 127, 1)]
NETWORK_SHAPES = [(64, 400, 400), (128, 200, 200), (256, 100, 100)]
_ENGINES = {}
_CASES = {}


def engine(max_batch=3):
    """An engine without weights (pp_unit_backward_mp is stateless and takes its map size from the call)."""
    if max_batch not in _ENGINES:
        load_pkg().install()
        _ENGINES[max_batch] = load_pkg("engine").Engine(small_cfg(24, 16, max_batch))
    return _ENGINES[max_batch]


def random_case(C, h, w, nb, seed):
    """Inputs of a case, generated once and shared by the tests that use it (never modified)."""
    key = (C, h, w, nb, seed)
    if key not in _CASES:
        rng = np.random.default_rng(seed)
        u = R.tie_free(rng.standard_normal((nb, C, h, w)))
        assert not R.near_ties(u, 1e-4).any()
        wt = (rng.standard_normal((C, C, 3, 3)) * 0.05).astype(np.float32)
        dz = rng.standard_normal((nb, C, h, w)).astype(np.float32)
        dskip = rng.standard_normal((nb, C, h, w)).astype(np.float32)
        _CASES[key] = (u, wt, dz, dskip)
    return _CASES[key]


# ------------------------------------------------------------------ 1. mode 0 is the old call
def test_fp32_mode_is_the_old_call():
    C, h, w, nb = 128, 20, 18, 2
    eng = engine()
    u, wt, dz, dskip = random_case(C, h, w, nb, 100 + C + h)
    ud, wd, dzd, dsd = dev(u), dev(wt), dev(dz), dev(dskip)
    old = eng.unit_backward(ud, wd, dzd, dskip=dsd)
    new = eng.unit_backward(ud, wd, dzd, dskip=dsd, grad_precision="fp32")
    assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1])
    dw, du = torch.empty_like(wd), torch.empty_like(ud)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for out in (dw, du):
        out.fill_(float("nan"))
    assert eng.lib.pp_unit_backward(eng.ctx, C, h, w, p(ud), p(wd), p(dzd), p(dsd), nb, p(dw), p(du), None) == 0  # the C entry itself
    torch.cuda.synchronize()
    assert torch.equal(dw, new[0]) and torch.equal(du, new[1])
    assert eng.unit_backward_path("fp32", C, h, w) == "fp32"


# ------------------------------------------------------------------ 2. shapes, both modes
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C,h,w,nb", SHAPES)
def test_shapes(C, h, w, nb, mode):
    eng = engine()
    assert eng.unit_backward_path(mode, C, h, w) == mode
    u, wt, dz, dskip = random_case(C, h, w, nb, 100 + C + h)
    ud, wd, dzd, dsd = dev(u), dev(wt), dev(dz), dev(dskip)
    dw, du = eng.unit_backward(ud, wd, dzd, grad_precision=mode)
    rw, ru, bw, bu, ties = M.grad_bounds_mixed(u, wt, dz, mode)
    assert not ties.any()
    check_bound(dw, rw, bw, f"{mode} {C}x{h}x{w}x{nb} dw")
    check_bound(du, ru, bu, f"{mode} {C}x{h}x{w}x{nb} du")
    dw2, du2 = eng.unit_backward(ud, wd, dzd, grad_precision=mode)
    dw3, none = eng.unit_backward(ud, wd, dzd, need_du=False, grad_precision=mode)
    assert none is None and torch.equal(dw, dw2) and torch.equal(du, du2) and torch.equal(dw, dw3)
    dw4, du4 = eng.unit_backward(ud, wd, dzd, dskip=dsd, grad_precision=mode)
    assert torch.equal(dw, dw4) and torch.equal(du4, du + dsd)  # dskip is exactly one fp32 add
    rw, ru, bw, bu, _ = M.grad_bounds_mixed(u, wt, dz, mode, dskip=dskip)
    check_bound(du4, ru, bu, f"{mode} {C}x{h}x{w}x{nb} du + dskip")


# ------------------------------------------------------------------ 3. the 16-bit path really ran
def test_path_query():
    eng = engine()
    for mode in MODES:
        for C, h, w in [s[:3] for s in SHAPES] + NETWORK_SHAPES:
            assert eng.unit_backward_path(mode, C, h, w) == mode, (mode, C, h, w)
    # 640 x 640 at C = 64: the hi and lo images of one frame pass the 256 MB budget (fp32 and plain bf16 fit): the fp32 kernels run
    assert eng.unit_backward_path("bf16x3", 64, 640, 640) == "fp32" and eng.unit_backward_path("bf16", 64, 640, 640) == "bf16"
    with pytest.raises(ValueError):
        eng.unit_backward_path("fp8", 64, 10, 10)
    with pytest.raises(RuntimeError):
        eng.unit_backward_path("bf16", 96, 10, 10)
    with pytest.raises(RuntimeError):
        eng.unit_backward_path("bf16", 64, 1, 1)
    assert eng.lib.pp_unit_backward_path(eng.ctx, 3, 64, 10, 10) < 0 and eng.lib.pp_unit_backward_path(eng.ctx, -1, 64, 10, 10) < 0


def test_modes_are_told_apart():
    C, h, w, nb = 64, 33, 17, 1
    eng = engine()
    u, wt, dz, _ = random_case(C, h, w, nb, 100 + C + h)
    rw, _, bw, _, _ = R.grad_bounds(u, wt, dz)
    err = {}
    for mode in MODES:
        dw, _ = eng.unit_backward(dev(u), dev(wt), dev(dz), grad_precision=mode)
        err[mode] = np.abs(dw.cpu().numpy().astype(np.float64) - rw)
    over = float((err["bf16"] / bw).max())
    gap = float(err["bf16"].max() / err["bf16x3"].max())
    print(f"bf16 dw: {over:.1f} x the fp32 bound at its worst element; largest deviation bf16 / bf16x3 = {gap:.0f}")
    assert over > 1.0                                      # no fp32 kernel does that
    assert err["bf16x3"].max() < err["bf16"].max() / 16.0  # and the split form is far closer: it is not the plain one either


# ------------------------------------------------------------------ 4. frames
@pytest.mark.parametrize("mode", MODES)
def test_frames(mode):
    C, h, w, nb = 128, 12, 10, 2
    eng = engine()
    u, wt, dz, dskip = random_case(C, h, w, nb, 7)
    dw, du = eng.unit_backward(dev(u), dev(wt), dev(dz), dskip=dev(dskip), grad_precision=mode)
    total = np.zeros(wt.shape)
    bound = M.grad_bounds_mixed(u, wt, dz, mode)[2]
    for f in range(nb):
        s = slice(f, f + 1)
        dwf, duf = eng.unit_backward(dev(u[s]), dev(wt), dev(dz[s]), dskip=dev(dskip[s]), grad_precision=mode)
        assert torch.equal(duf[0], du[f]), f  # a frame's du does not depend on the batch it rides in
        total += dwf.cpu().numpy().astype(np.float64)
        bound = bound + M.grad_bounds_mixed(u[s], wt, dz[s], mode)[2]
    check_bound(dw, total, bound, f"{mode} frames dw")


# ------------------------------------------------------------------ 5. autograd surface
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
    calls = []
    inner = eng.unit_backward

    def recording(u, w, dy, dskip=None, need_du=True, grad_precision="fp32"):
        out = inner(u, w, dy, dskip=dskip, need_du=need_du, grad_precision=grad_precision)
        calls.append((w, u, dy, grad_precision, out[0]))
        return out

    monkeypatch.setattr(eng, "unit_backward", recording)

    def grads_of(**kw):
        net.train(scope="rpn", **kw)
        preds = net(example)
        for k in plain:
            assert torch.equal(preds[k].detach(), plain[k]), k  # the training forward stays fp32: the inference bits
        net.zero_grad()
        del calls[:]
        sum((preds[k] * up[k]).sum() for k in preds).backward()
        return {k: p.grad.clone() for k, p in net.named_parameters()}, list(calls)

    base, base_calls = grads_of()
    assert net.grad_precision == "fp32" and len(base) == 25 and len(base_calls) == 13
    assert all(c[3] == "fp32" for c in base_calls)
    explicit, _ = grads_of(grad_precision="fp32")
    for k in base:
        assert torch.equal(base[k], explicit[k]), k
    units = [k for k in shared.RPN_CONV_KEYS if k not in eng.DOWN_KEYS]
    assert len(units) == 13
    for mode in MODES:
        got, seen = grads_of(grad_precision=mode)
        assert net.grad_precision == mode
        assert len(seen) == 13 and all(c[3] == mode for c in seen)  # every unit backward of the chain got the keyword
        params = dict(net.named_parameters())
        by_weight = {c[0].data_ptr(): c for c in seen}
        for k in shared.HEAD_KEYS:  # what runs in front of the first unit backward did not change
            assert torch.equal(got[k], base[k]), k
        moved = 0
        for k in units:
            _, u, dy, _, dw = by_weight[params[k].data_ptr()]
            assert torch.equal(dw, got[k]), k  # what the call returned is what autograd delivered
            moved += int(not torch.equal(got[k], base[k]))
            rw, _, bw, _, ties = M.grad_bounds_mixed(u.cpu().numpy(), params[k].detach().cpu().numpy(), dy.cpu().numpy(), mode)
            assert ties.sum() <= 1e-3 * ties.size, k
            check_bound(dw, rw, bw, f"{mode} autograd dw {k}")
        assert moved == 13, moved
    with pytest.raises(ValueError):
        net.train(grad_precision="fp8")
    net.train(scope="neck", grad_precision="bf16")  # accepted and inert
    assert net.grad_precision == "bf16"
    net.eval()
    assert net.grad_precision == "fp32"
    again, _ = grads_of()
    for k in base:
        assert torch.equal(base[k], again[k]), k


# ------------------------------------------------------------------ 6. it trains
@pytest.mark.parametrize("mode", MODES)
def test_it_trains(mode):
    """Twenty Adam steps (lr 1e-3, clip_grad_norm_ 10) on a fixed batch of two frames under scope "rpn".  A sanity condition, not a
    measurement: fp32 ends at 6 % of the initial loss (0.0976 from 1.5557), and a mode that cannot halve it is not training."""
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
    net.train(scope="rpn", grad_precision=mode)
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
    print(mode, " ".join(f"{v:.6f}" for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < 0.5 * losses[0], (mode, losses)


# ------------------------------------------------------------------ 7. errors
def test_bad_arguments_raise_and_the_next_call_works():
    _lib = load_pkg("_lib")
    eng = engine()
    C, h, w, nb = 64, 9, 7, 2
    u, wt, dz, dskip = random_case(C, h, w, nb, 5)
    ud, wd, dzd = dev(u), dev(wt), dev(dz)
    good = eng.unit_backward(ud, wd, dzd, grad_precision="bf16")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dw, du = torch.empty_like(wd), torch.empty_like(ud)

    def call(mode, C=C, wptr=None):
        rc = eng.lib.pp_unit_backward_mp(eng.ctx, mode, C, h, w, p(ud), wptr or p(wd), p(dzd), None, nb, p(dw), p(du), None)
        _lib.check(rc, eng.ctx, "pp_unit_backward_mp")

    for mode in (3, -1):
        with pytest.raises(RuntimeError, match="mode"):
            call(mode)
    for mode in (0, 1, 2):
        with pytest.raises(RuntimeError, match="64, 128 or 256"):
            call(mode, C=96)
        with pytest.raises(RuntimeError, match="aligned"):
            call(mode, wptr=ctypes.c_void_p(wd.data_ptr() + 4))
    with pytest.raises(ValueError):
        eng.unit_backward(ud, wd, dzd, grad_precision="fp16")
    with pytest.raises(ValueError):
        eng.unit_backward(ud, wd, dzd, grad_precision=2)
    call(2)
    torch.cuda.synchronize()
    assert torch.equal(dw, good[0]) and torch.equal(du, good[1])
    again = eng.unit_backward(ud, wd, dzd, grad_precision="bf16")
    assert torch.equal(again[0], good[0]) and torch.equal(again[1], good[1])
