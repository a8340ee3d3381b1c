"""CPU: the float64 restatement of the strided stage (tests/downtrain_ref.py) against the reference's float64 autograd goldens
(tests/golden/downtrain_small.npz, tests/golden/make_downtrain_goldens.py), the fixture's freedom from ReLU near-ties, the a-priori
bounds against a float32 evaluation with shuffled summation order, and a resource audit of csrc/down_train.hip (no GPU needed: hipcc
cross-compiles for gfx950): no kernel of the stage backward may spill."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, golden
import downtrain_ref as R
from test_head_deferred_isa_cpu import HIPCC, kernel_usage

sys.path.insert(0, GOLDEN)
from make_downtrain_goldens import DW_STRIDE, MODULES, SEEDS, TIE, small_inputs  # noqa: E402


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("name", list(MODULES))
def test_restatement_matches_the_reference(name):
    g = golden("downtrain_small")
    x, w, dy = small_inputs(name)
    assert int(g["seed_" + name]) == SEEDS[name]
    h, z = R.down_forward(x, w, return_z=True)
    dw, dx = R.down_backward(x, w, z, dy)
    assert dx.shape == x.shape and dw.shape == w.shape
    assert rel(dx, g["dx_" + name]) <= 1e-12
    assert rel(dw.reshape(-1)[::DW_STRIDE[name]], g["dw_" + name]) <= 1e-12
    assert abs(np.abs(dw).max() - float(g[f"dw_{name}_max"])) <= 1e-12 * np.abs(dw).max()
    # the stored conv output is the float32 run's: its own rounding away from the float64 forward
    assert g["z_" + name].dtype == np.float32 and rel(z, g["z_" + name].astype(np.float64)) <= 1e-5
    assert h.min() >= 0 and np.array_equal(h > 0, R.norm(z)[0] > 0)


@pytest.mark.parametrize("name", list(MODULES))
def test_fixture_has_no_near_tie(name):
    g = golden("downtrain_small")
    x, w, _ = small_inputs(name)
    assert not R.near_ties(R.down_forward(x, w, return_z=True)[1], TIE).any()
    assert not R.near_ties(g["z_" + name], TIE).any()


def test_dgrad_tap_counts_follow_parity():
    """With unit weights and unit dz, dx counts the taps an input pixel is seen through: 1, 2, 2 or 4 by parity, fewer at an even
    size's last row / column (ky = 0 would point at oy = ho)."""
    for hin, win in ((6, 5), (1, 4), (2, 3)):
        ho, wo = R.out_size(hin, win)
        cnt = R.conv_s2_dgrad(np.ones((1, 1, ho, wo)), np.ones((1, 1, 3, 3)), hin, win)[0, 0]
        ny = np.array([1 if y % 2 == 0 else (1 if y == hin - 1 and hin % 2 == 0 else 2) for y in range(hin)])
        nx = np.array([1 if x % 2 == 0 else (1 if x == win - 1 and win % 2 == 0 else 2) for x in range(win)])
        assert np.array_equal(cnt, np.outer(ny, nx)), (hin, win)


def test_bounds_hold_for_a_float32_evaluation():
    """grad_bounds against a numpy float32 evaluation of the same formulas whose two products add their terms one by one in a
    shuffled order: inside, and not vacuous."""
    rng = np.random.default_rng(5)
    f = np.float32
    nb, cin, cout, hin, win = 2, 6, 8, 7, 6
    x = rng.standard_normal((nb, cin, hin, win)).astype(f)
    w = (rng.standard_normal((cout, cin, 3, 3)) * 0.05).astype(f)
    z = R.tie_free(R.conv_s2(x.astype(np.float64), w.astype(np.float64)))
    ho, wo = z.shape[-2:]
    dy = rng.standard_normal(z.shape).astype(f)
    dw, dx, bw, bx, ties = R.grad_bounds(x, w, z, dy)
    assert not ties.any()
    mean = z.astype(np.float64).mean((2, 3), keepdims=True)
    rstd = 1.0 / np.sqrt(z.astype(np.float64).var((2, 3), keepdims=True) + R.EPS)
    xhat = (z - mean.astype(f)) * rstd.astype(f)
    Gr = np.where(xhat > 0, dy, f(0))
    c1 = Gr.astype(np.float64).mean((2, 3), keepdims=True).astype(f)
    c2 = (Gr.astype(np.float64) * xhat).mean((2, 3), keepdims=True).astype(f)
    dz = rstd.astype(f) * ((Gr - c1) - xhat * c2)
    assert dz.dtype == f
    # dw: the K = nb ho wo products of every element, added in float32 in a shuffled order
    dw32 = np.empty(w.shape, f)
    for ky in range(3):
        for kx in range(3):
            terms = (dz[:, :, None] * R.tap_view(x, ky, kx)[:, None]).transpose(0, 3, 4, 1, 2).reshape(nb * ho * wo, cout, cin)
            dw32[:, :, ky, kx] = np.cumsum(terms[rng.permutation(len(terms))], axis=0, dtype=f)[-1]
    # dx: the (co, ky, kx) products of every element (zero where a tap does not reach it), likewise
    terms = np.zeros((cout, 9, nb, cin, hin + 3, win + 3), f)
    for ky in range(3):
        for kx in range(3):
            terms[:, ky * 3 + kx, :, :, ky:ky + 2 * ho - 1:2, kx:kx + 2 * wo - 1:2] = \
                (w[:, :, ky, kx][:, None, :, None, None] * dz.transpose(1, 0, 2, 3)[:, :, None]).astype(f)
    terms = terms.reshape(cout * 9, nb, cin, hin + 3, win + 3)[..., 1:1 + hin, 1:1 + win]
    dx32 = np.cumsum(terms[rng.permutation(len(terms))], axis=0, dtype=f)[-1]
    fw, fx = np.abs(dw32 - dw) / bw, np.abs(dx32 - dx) / bx
    print("fractions of the bounds:", fw.max(), fx.max())
    assert fw.max() <= 1.0 and fx.max() <= 1.0
    assert bw.max() <= 1e-3 * np.abs(dw).max() and bx.max() <= 1e-3 * np.abs(dx).max()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_down_backward_kernels_use_no_scratch():
    k = {n: u for n, u in kernel_usage("down_train.hip").items() if "k_down_" in n or "k_conv3_" in n or "k_dw_reduce" in n}
    print(k)
    # conv3_wt and conv3_wgrad<2 | 4> (train_conv3.h's, shared with the Resnet unit), xpack, norm, dw_reduce (train_host.h's, shared by
    # the three families), dgrad<1 | 2>
    assert len(k) == 8, sorted(k)
    for n, u in k.items():
        assert u["ScratchSize [bytes/lane]"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (n, u)
