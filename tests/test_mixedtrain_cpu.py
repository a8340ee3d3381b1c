"""CPU: the numpy side of the mixed-precision unit backward (tests/mixedtrain_ref.py): bf16 rounding and splitting, and the emulated
arithmetic of both modes against the a-priori bounds the GPU tests use.  The emulation keeps products and sums in float64, so what it
shows is that the operand terms of the bounds hold and are not vacuous; the fp32 accumulation terms are the GPU tests' business."""
import os

import numpy as np
import pytest

from test_head_deferred_isa_cpu import HIPCC, kernel_usage
import blocktrain_ref as R
import mixedtrain_ref as M

CASES = [(64, 9, 7, 2), (128, 12, 10, 2)]


def random_case(C, h, w, nb, seed):
    rng = np.random.default_rng(seed)
    u = R.tie_free(rng.standard_normal((nb, C, h, w)))
    wt = (rng.standard_normal((C, C, 3, 3)) * 0.05).astype(np.float32)
    dz = rng.standard_normal((nb, C, h, w)).astype(np.float32)
    dskip = rng.standard_normal((nb, C, h, w)).astype(np.float32)
    return u, wt, dz, dskip


def test_bf16_round_ties_to_even():
    f = lambda bits: np.array([bits], np.uint32).view(np.float32)  # noqa: E731
    assert M.bf16_round(f(0x3F808000))[0] == f(0x3F800000)[0]  # 1 + 2^-8: halfway, the even neighbour is below
    assert M.bf16_round(f(0x3F818000))[0] == f(0x3F820000)[0]  # halfway, the even neighbour is above
    assert M.bf16_round(f(0x3F808001))[0] == f(0x3F810000)[0]  # just above halfway
    assert M.bf16_round(f(0x3F807FFF))[0] == f(0x3F800000)[0]  # just below
    assert M.bf16_round(f(0xBF808000))[0] == f(0xBF800000)[0]  # the sign does not matter
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    r = M.bf16_round(x)
    assert (r.view(np.uint32) & 0xFFFF == 0).all() and (np.abs(r.astype(np.float64) - x) <= M.U16 * np.abs(x)).all()
    assert np.array_equal(M.bf16_round(r), r) and M.bf16_round(np.zeros(1, np.float32))[0] == 0


def test_split_reconstructs():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(1 << 16) * np.exp(rng.uniform(-20, 20, 1 << 16))).astype(np.float32)
    hi, lo = M.bf16_split(x)
    assert (hi.view(np.uint32) & 0xFFFF == 0).all() and (lo.view(np.uint32) & 0xFFFF == 0).all()
    err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - x.astype(np.float64))
    assert (err <= 2.0 ** -16 * np.abs(x)).all()
    pos = x[x > 0]
    assert (M.bf16_round(pos) > 0).all()  # a positive normal float32 never rounds to 0: the bf16 a image carries fp32's mask


def test_restated_bounds_are_grad_bounds():
    """eps = 0, m = 1: the restatement in mixedtrain_ref is blocktrain_ref.grad_bounds, with and without dskip."""
    u, wt, dz, dskip = random_case(64, 9, 7, 2, 11)
    u[0, 3, 4, 2] = u[0, 3].mean()  # a near-tie, so that the jump terms are compared too
    for ds in (None, dskip):
        want = R.grad_bounds(u, wt, dz, dskip=ds, tie=1e-2)
        got = M._bounds(u, wt, dz, ds, 1e-2, 0.0, 1)
        assert want[4].any() and np.array_equal(want[4], got[4])
        for a, b in zip(want[:4], got[:4]):
            assert np.allclose(a, b, rtol=1e-9, atol=1e-12 * np.abs(a).max())  # the sums run in another order
    plain = R.grad_bounds(u, wt, dz)
    for mode in M.MODES:
        mixed = M.grad_bounds_mixed(u, wt, dz, mode)
        assert (mixed[2] > plain[2]).all() and (mixed[3] >= plain[3] * (1 - 1e-9)).all() and (mixed[3] > plain[3]).any()


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("C,h,w,nb", CASES)
def test_emulation_within_bounds(C, h, w, nb, mode):
    u, wt, dz, dskip = random_case(C, h, w, nb, 300 + C + h)
    rw, ru, bw, bu, ties = M.grad_bounds_mixed(u, wt, dz, mode, dskip=dskip)
    assert not ties.any()
    dw, du = M.emulate(u, wt, dz, mode, dskip=dskip)
    fw, fu = float((np.abs(dw - rw) / bw).max()), float((np.abs(du - ru) / bu).max())
    rel = float(np.abs(dw - rw).max() / np.abs(rw).max())
    plain = R.grad_bounds(u, wt, dz, dskip=dskip)[2]
    over = float((np.abs(dw - rw) / plain).max())
    print(f"{mode} {C}x{h}x{w}x{nb}: dw {fw:.3f} of bw_mixed, du {fu:.3f} of bu_mixed, dw error / max|dw| {rel:.2e}, {over:.2f} x the fp32 bw")
    assert fw <= 1.0 and fu <= 1.0
    assert fw > 1e-3 and fu > 1e-3  # not vacuous
    if mode == "bf16":
        assert over > 1.0  # plain bf16 is outside what an fp32 implementation may do: the GPU test tells the paths apart by this


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_mixed_kernels_use_no_scratch():
    k = {n: u for n, u in kernel_usage("block_train16.hip").items() if "16" in n or n.endswith("_u") or "_uE" in n}
    # per mode: wt16, pack16, packT16, wgrad16 x 2 tilings, dgrad16 x 3 widths
    assert sum("wgrad16" in n for n in k) == 4 and sum("dgrad16" in n for n in k) == 6 and len(k) >= 16, sorted(k)
    for n, u in k.items():
        assert u["ScratchSize [bytes/lane]"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (n, u)
