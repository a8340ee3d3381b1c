"""CPU: the float64 restatement of the Resnet unit (tests/blocktrain_ref.py) against the reference's float64 autograd goldens
(tests/golden/blocktrain_small.npz, tests/golden/make_blocktrain_goldens.py), the fixture's freedom from ReLU near-ties, and a
resource audit of csrc/block_train.hip (no GPU needed: hipcc cross-compiles for gfx950): no kernel of the unit backward may spill."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, golden
import blocktrain_ref as R
from test_head_deferred_isa_cpu import HIPCC, kernel_usage

sys.path.insert(0, GOLDEN)
from make_blocktrain_goldens import DW_STRIDE, MODULES, SEEDS, TIE, UNITS, restated, small_inputs  # noqa: E402


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("name", list(MODULES))
def test_restatement_matches_the_reference(name):
    g = golden("blocktrain_small")
    x, ws, dy = small_inputs(name)
    us, dws, dx = restated(R, x, ws, dy)
    assert int(g["seed_" + name]) == SEEDS[name] and len(ws) == UNITS[name]
    assert rel(dx, g["dx_" + name]) <= 1e-12
    for k in range(len(ws)):
        assert rel(dws[k].reshape(-1)[::DW_STRIDE[name]], g[f"dw_{name}_{k}"]) <= 1e-12, k
        assert abs(np.abs(dws[k]).max() - float(g[f"dw_{name}_{k}_max"])) <= 1e-12 * np.abs(dws[k]).max()
        # the stored unit inputs are the float32 run's: its own rounding away from the float64 forward
        assert rel(us[k], g[f"u_{name}_{k}"].astype(np.float64)) <= 1e-5, k


@pytest.mark.parametrize("name", list(MODULES))
def test_fixture_has_no_near_tie(name):
    g = golden("blocktrain_small")
    x, ws, dy = small_inputs(name)
    for k, u in enumerate(restated(R, x, ws, dy)[0]):
        assert not R.near_ties(u, TIE).any(), k
        assert not R.near_ties(g[f"u_{name}_{k}"], TIE).any(), k


def test_bounds_hold_for_a_float32_evaluation():
    """grad_bounds against a plain numpy float32 evaluation of the same formulas (sums in numpy's order): inside, and not vacuous."""
    rng = np.random.default_rng(5)
    u = R.tie_free(rng.standard_normal((2, 8, 5, 4)))
    w = (rng.standard_normal((8, 8, 3, 3)) * 0.05).astype(np.float32)
    dz = rng.standard_normal((2, 8, 5, 4)).astype(np.float32)
    dw, du, bw, bu, ties = R.grad_bounds(u, w, dz, dskip=dz)
    assert not ties.any()
    f = np.float32
    mean = u.astype(np.float64).mean((2, 3), keepdims=True)
    rstd = 1.0 / np.sqrt(u.astype(np.float64).var((2, 3), keepdims=True) + R.EPS)
    xhat = (u - mean.astype(f)) * rstd.astype(f)
    a = np.maximum(xhat, f(0))
    dw32 = R.conv3_wgrad(dz, a).astype(f)
    Gr = (R.conv3_dgrad(dz, w).astype(f) * (a > 0)).astype(f)
    c1 = Gr.astype(np.float64).mean((2, 3), keepdims=True).astype(f)
    c2 = (Gr.astype(np.float64) * xhat).mean((2, 3), keepdims=True).astype(f)
    du32 = rstd.astype(f) * ((Gr - c1) - xhat * c2) + dz
    assert du32.dtype == f
    fw, fu = np.abs(dw32 - dw) / bw, np.abs(du32 - du) / bu
    print("fractions of the bounds:", fw.max(), fu.max())
    assert fw.max() <= 1.0 and fu.max() <= 1.0
    assert bw.max() <= 1e-3 * np.abs(dw).max() and bu.max() <= 1e-3 * np.abs(du).max()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_unit_backward_kernels_use_no_scratch():
    k = {n: u for n, u in kernel_usage("block_train.hip").items() if "k_unit_" in n or "k_conv3_" in n or "k_dw_reduce" in n}
    print(k)
    # conv3_wt and conv3_wgrad<2 | 4> (train_conv3.h's, shared with the strided stage), pack, dw_reduce (train_host.h's, shared by the
    # three families), dgrad<1 | 2 | 4>, norm, image
    assert len(k) == 10, sorted(k)
    for n, u in k.items():
        assert u["ScratchSize [bytes/lane]"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (n, u)
