"""CPU: the float64 restatement of training the BatchNorm RPN with batch statistics (tests/bnbatch_ref.py) -- the three backward
primitives against torch autograd on the CPU in float64 (BatchNorm in training mode), the whole chain, the forward, the batch
statistics and the moved running statistics against the reference's float64 goldens (tests/golden/bnbatch_small.npz,
tests/golden/make_bnbatch_goldens.py) -- and, on a network object assembled without an engine, the scope and argument rules of
train(bn_stats="moving").  Also the C ABI's declarations and a resource audit of the new streaming kernels."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, golden, load_pkg
import blocktrain_ref as B
import bnbatch_ref as R
from test_bntrain_cpu import engineless, norm_params, rel, t64
from test_head_deferred_isa_cpu import HIPCC, kernel_usage

sys.path.insert(0, GOLDEN)
from make_bnbatch_goldens import BN_C, DW_STRIDE, DX_STRIDE, SEED, Y_STRIDE, small_inputs, split  # noqa: E402

SYMBOLS = ("pp_backbone_train_taps_bn", "pp_unit_backward_bn", "pp_down_backward_bn", "pp_neck_backward_bn")


def bn_train(v, gamma, beta):
    return torch.nn.functional.batch_norm(v, None, None, gamma, beta, training=True, eps=1e-3)


def folded(v, bn):
    """Batch statistics of v and their fold with (gamma, beta), float64."""
    mean, var = R.batch_stats(v)
    return (*R.fold(bn[0], bn[1], mean, var), mean, var)


# ------------------------------------------------------------------ 1. the primitives against torch autograd
@pytest.mark.parametrize("C,h,w,nb,skip", [(64, 7, 5, 2, True), (128, 3, 2, 3, False)])
def test_unit_against_autograd(C, h, w, nb, skip):
    rng = np.random.default_rng(C + h)
    u, wt, dz = rng.standard_normal((nb, C, h, w)), rng.standard_normal((C, C, 3, 3)) * 0.05, rng.standard_normal((nb, C, h, w))
    bn = norm_params(rng, C)
    ut, wtt, gamma, beta = t64(u, True), t64(wt, True), t64(bn[0], True), t64(bn[1], True)
    z = torch.nn.functional.conv2d(torch.relu(bn_train(ut, gamma, beta)), wtt, padding=1)
    (z + ut if skip else z).backward(t64(dz))
    scale, shift, mean, var = folded(u, bn)
    assert rel(R.unit_forward(u, wt, scale, shift), z.detach().numpy()) <= 1e-10
    dw, du, ds, dh = R.unit_backward(u, wt, scale, shift, mean, var, dz, dskip=dz if skip else None)
    dg, db = R.affine_grad(ds, dh, mean, var)
    for name, got, want in (("dw", dw, wtt.grad), ("du", du, ut.grad), ("dgamma", dg, gamma.grad), ("dbeta", db, beta.grad)):
        assert rel(got, want.numpy()) <= 1e-10, name


@pytest.mark.parametrize("cin,cout,hin,win", [(64, 64, 6, 4), (64, 128, 5, 3)])
def test_down_against_autograd(cin, cout, hin, win):
    rng = np.random.default_rng(cin + cout + hin)
    ho, wo = (hin + 1) // 2, (win + 1) // 2
    x, wt, dy = rng.standard_normal((2, cin, hin, win)), rng.standard_normal((cout, cin, 3, 3)) * 0.05, rng.standard_normal((2, cout, ho, wo))
    bn = norm_params(rng, cout)
    xt, wtt, gamma, beta = t64(x, True), t64(wt, True), t64(bn[0], True), t64(bn[1], True)
    zt = torch.nn.functional.conv2d(xt, wtt, stride=2, padding=1)
    ht = torch.relu(bn_train(zt, gamma, beta))
    ht.backward(t64(dy))
    z = R.D.conv_s2(x, wt)
    scale, shift, mean, var = folded(z, bn)
    assert rel(R.down_forward(x, wt, scale, shift), ht.detach().numpy()) <= 1e-10 and rel(z, zt.detach().numpy()) <= 1e-10
    dw, dx, ds, dh = R.down_backward(x, wt, z, scale, shift, mean, var, dy)
    dg, db = R.affine_grad(ds, dh, mean, var)
    for name, got, want in (("dw", dw, wtt.grad), ("dx", dx, xt.grad), ("dgamma", dg, gamma.grad), ("dbeta", db, beta.grad)):
        assert rel(got, want.numpy()) <= 1e-10, name


@pytest.mark.parametrize("branch", [0, 1, 2])
def test_branch_against_autograd(branch):
    rng = np.random.default_rng(40 + branch)
    cin, cup, s, h, w = R.N.CIN[branch], R.N.CUP[branch], 1 << branch, 3, 2
    x, wt, dy = rng.standard_normal((2, cin, h, w)), rng.standard_normal((cin, cup, s, s)) * 0.05, rng.standard_normal((2, cup, s * h, s * w))
    bn = norm_params(rng, cup)
    xt, wtt, gamma, beta = t64(x, True), t64(wt, True), t64(bn[0], True), t64(bn[1], True)
    yt = torch.relu(bn_train(torch.nn.functional.conv_transpose2d(xt, wtt, stride=s), gamma, beta))
    yt.backward(t64(dy))
    scale, shift, mean, var = folded(R.N.conv_t(x, wt), bn)
    y = R.branch_forward(x, wt, scale, shift)
    assert rel(y, yt.detach().numpy()) <= 1e-10
    dw, dx, ds, dh = R.branch_backward(x, wt, scale, mean, var, y, dy)
    dg, db = R.affine_grad(ds, dh, mean, var)
    for name, got, want in (("dw", dw, wtt.grad), ("dx", dx, xt.grad), ("dgamma", dg, gamma.grad), ("dbeta", db, beta.grad)):
        assert rel(got, want.numpy()) <= 1e-10, name


def test_one_frame_without_affine_is_instance_norm():
    """Train-mode BatchNorm of one frame with gamma = 1, beta = 0 is InstanceNorm: the restatement equals blocktrain_ref's unit."""
    rng = np.random.default_rng(5)
    C, h, w = 64, 6, 5
    u, wt, dz, dskip = (rng.standard_normal(s) for s in ((1, C, h, w), (C, C, 3, 3), (1, C, h, w), (1, C, h, w)))
    scale, shift, mean, var = folded(u, (np.ones(C), np.zeros(C)))
    for skip in (None, dskip):
        dw, du, _, _ = R.unit_backward(u, wt, scale, shift, mean, var, dz, dskip=skip)
        rw, ru = B.unit_backward(u, wt, dz, dskip=skip)
        assert rel(dw, rw) <= 1e-12 and rel(du, ru) <= 1e-12


def test_bounds_hold_for_a_float32_evaluation():
    """The a-priori bounds are not vacuous and not violated: a numpy float32 evaluation of the unit's formulas lies inside them."""
    rng = np.random.default_rng(6)
    C, h, w, nb = 64, 5, 4, 2
    u = rng.standard_normal((nb, C, h, w)).astype(np.float32)
    wt = (rng.standard_normal((C, C, 3, 3)) * 0.05).astype(np.float32)
    dz = rng.standard_normal((nb, C, h, w)).astype(np.float32)
    mean, var = R.stats32(u)
    scale, shift = R.fold32(*norm_params(rng, C)[:2], mean, var)
    (dw, du, ds, dh), (bw, bu, bs, bh) = R.unit_bounds(u, wt, scale, shift, mean, var, dz)
    f = np.float32
    a = np.maximum(u * scale[None, :, None, None] + shift[None, :, None, None], f(0))
    g = (B.conv3_dgrad(dz.astype(np.float64), wt.astype(np.float64)).astype(f) * (a > 0)).astype(f)
    n = nb * h * w
    s, q = g.astype(np.float64).sum((0, 2, 3)), (g.astype(np.float64) * u).sum((0, 2, 3))
    r = 1.0 / np.sqrt(var.astype(np.float64) + R.EPS)
    c1, c2 = (s / n).astype(f), (r * (q - mean.astype(np.float64) * s) / n).astype(f)
    xhat = ((u - R.ch(mean).astype(f)) * R.ch(r).astype(f)).astype(f)
    du32 = (R.ch(scale).astype(f) * ((g - R.ch(c1).astype(f)) - xhat * R.ch(c2).astype(f))).astype(f)
    assert du32.dtype == np.float32 and (np.abs(du32 - du) <= bu).all()
    assert (np.abs(s - dh) <= bh).all() and (np.abs(q - ds) <= bs).all()
    # not vacuous: the dgrad's 9 C = 576 terms dominate, 576 U ~ 3.4e-5 of sum |w dz|, a few times |du|
    assert np.median(bu / np.abs(du).max()) < 1e-3 and (bw < 1e-3 * np.abs(dw).max()).all()


# ------------------------------------------------------------------ 2. the chain against the reference
@pytest.fixture(scope="module")
def restated():
    canvas, ws, bn, dy = small_inputs()
    wc, wn = split(ws)
    bnd = dict(zip(R.BN_PREFIXES, bn))
    fwd = R.rpn_forward(canvas, wc, wn, bnd)
    grads, dx = R.rpn_backward(canvas, wc, wn, bnd, fwd, dy)
    return dict(fwd=fwd, grads=grads, dx=dx, ws=ws, bn=bn)


def test_restatement_matches_the_reference(restated):
    g = golden("bnbatch_small")
    assert int(g["seed"]) == SEED == 11 and int(g["dw_stride"]) == DW_STRIDE and int(g["dx_stride"]) == DX_STRIDE and int(g["y_stride"]) == Y_STRIDE
    names = [str(k) for k in g["param_names"]]
    assert names == list(R.PARAM_KEYS) and len(names) == 57 and [t[0].shape[0] for t in restated["bn"]] == list(BN_C)
    for i, k in enumerate(names):
        got = restated["grads"][k]
        got = got.reshape(-1)[::DW_STRIDE] if got.ndim == 4 else got
        assert got.shape == g[f"g_{i}"].shape and rel(got, g[f"g_{i}"]) <= 1e-10, k
    assert rel(restated["dx"].reshape(-1)[::DX_STRIDE], g["dcanvas"]) <= 1e-10
    fwd = restated["fwd"]
    assert rel(fwd["y"].reshape(-1)[::Y_STRIDE], g["rpn_out"]) <= 1e-10
    for i, (p, t) in enumerate(zip(R.BN_PREFIXES, restated["bn"])):
        mean, var, n = fwd["stats"][p]
        assert rel(mean, g[f"mean_{i}"]) <= 1e-10 and rel(var, g[f"var_{i}"]) <= 1e-10, p
        rm, rv = R.moved(t[2], t[3], mean, var, n)
        assert rel(rm, g[f"rm_{i}"]) <= 1e-10 and rel(rv, g[f"rv_{i}"]) <= 1e-10, p
    # the reference's own float32 deviations the GPU bars are taken from
    assert max(float(g[f"ref32_dev_g_{i}"]) for i in range(57)) < 5e-6 and float(g["ref32_dev_dcanvas"]) < 3e-6
    assert float(g["ref32_abs_rpn_out"]) < 2e-5 and float(g["ref32_abs_running"]) < 3e-7


def test_fixture_masks(restated):
    """The mask condition of the seed: every ReLU takes both branches, and no pre-activation is so close to zero that a float32
    forward within the backbone bar could take the other one unnoticed (the generator asserts the reference's float32 run does not)."""
    fwd = restated["fwd"]
    masks = R.relu_masks(fwd)
    assert len(masks) == 19 and all(0 < m.mean() < 1 for m in masks.values())
    for b in range(3):
        assert np.array_equal(fwd["units"][b][0] > 0, masks[f"stage{b}"])
    assert [len(u) for u in fwd["units"]] == [3, 5, 5] and fwd["y"].shape == (2, 320, 16, 12) and len(fwd["stats"]) == 19


# ------------------------------------------------------------------ 3. scope and argument rules
def test_train_argument_rules():
    shared = load_pkg("networks.pointpillars8_shared")
    assert "moving" in shared.BN_STATS and shared.BN2D_MOMENTUM == R.MOMENTUM
    bn = engineless(load_pkg("networks.pointpillars8_export").PointPillars, shared)
    trt = engineless(load_pkg("networks.pointpillars8_trt").PointPillars, shared)
    inn = engineless(shared.PointPillars, shared)
    for net in (bn, trt):
        for scope, count in (("head", 6), ("neck", 15), ("block3", 30), ("stage3", 33), ("rpn", 63), ("all", 66)):
            assert net.train(scope=scope, bn_stats="moving") is net and net.bn_stats == "moving" and net.training
            assert len(list(net.parameters())) == count and all(p.requires_grad for p in net.parameters()), scope
        net.train(scope="rpn", bn_stats="moving")
        assert [k for k, _ in net.named_parameters()] == list(shared.BN_RPN_KEYS)
        assert net._neck_grad()  # the training forward runs the lock-step pass
        with torch.no_grad():
            assert net._neck_grad()  # ... whether or not grad is enabled: the running statistics move
        with pytest.raises(NotImplementedError, match="moving"):
            net.train(scope="rpn", bn_stats="batch")
        for prec in ("bf16x3", "bf16"):
            with pytest.raises(ValueError, match="fp32"):
                net.train(scope="rpn", bn_stats="moving", grad_precision=prec)
        net.eval()
        assert net.bn_stats is None and not net._neck_grad()
    with pytest.raises(ValueError, match="BatchNorm"):
        inn.train(scope="rpn", bn_stats="moving")


# ------------------------------------------------------------------ 4. ABI and resources
def test_c_abi_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    protos = load_pkg("_lib").PROTOTYPES
    for name in SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name + " is not declared in include/pp_hip.h"
        nargs = len([a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()])
        assert name in protos and len(protos[name][1]) == nargs, (name, nargs)
    eng = load_pkg("engine").Engine
    assert all(hasattr(eng, n) for n in ("backbone_train_taps_bn", "unit_backward_bn", "down_backward_bn", "neck_backward_bn"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src,names", [("block_train.hip", ("k_bn_plane_sums", "k_bn_unit_du", "k_bn_coef")),
                                       ("down_train.hip", ("k_bn_plane_sums", "k_bn_down_dz", "k_bn_coef")),
                                       ("neck_train.hip", ("k_bn_neck_sums", "k_bn_neck_dz", "k_bn_coef"))])
def test_bn_passes_use_no_scratch(src, names):
    k = {n: u for n, u in kernel_usage(src).items() if "k_bn_" in n}
    print(k)
    assert len(k) == len(names) and all(any(m in n for n in k) for m in names), sorted(k)
    for n, u in k.items():
        assert u["ScratchSize [bytes/lane]"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (n, u)
