"""CPU: the bounds and the emulation of tests/mixedstage_ref.py hold together on every input set tests/test_mixedstage_gpu.py uses, so
that a correct 16-bit kernel can meet every condition the GPU tests assert: the emulated arithmetic of a mode lies inside its a-priori
bound, the fp32 arithmetic with the same float32 dz inside the plain one, the seeded conv outputs have no near-tie of the ReLU, and
the "told apart" inputs separate the modes."""
import functools

import numpy as np
import pytest

import mixedstage_ref as M

MIXED = ("bf16x3", "bf16")


@functools.lru_cache(maxsize=None)
def down_set(shape):
    case = M.down_case(*shape)
    return case, M.down_terms(*case)


@functools.lru_cache(maxsize=None)
def neck_set(shape):
    xs, ws, y, dy = M.neck_case(*shape)
    cases = [(xs[b], ws[b], y[:, M.branch_slice(b)], dy[:, M.branch_slice(b)]) for b in range(3)]
    return cases, [M.neck_terms(*c) for c in cases]


@pytest.mark.parametrize("shape", M.DOWN_SHAPES + [M.DOWN_APART])
def test_down_emulation_inside_bounds(shape):
    case, t = down_set(shape)
    assert not t["ties"].any() and not M.D.near_ties(case[2], 1e-4).any()
    for mode in ("fp32",) + MIXED:
        dw, dx = M.down_emulate(*case, mode)
        rw, rx, bw, bx, _ = M.down_grad_bounds_mixed(*case, mode, terms=t)
        fw, fx = M.worst(dw, rw, bw)[0], M.worst(dx, rx, bx)[0]
        print(f"down {shape} {mode}: emulation at {fw:.3f} (dw), {fx:.3f} (dx) of the bound")
        assert fw <= 1.0 and fx <= 1.0, (shape, mode, fw, fx)


@pytest.mark.parametrize("shape", M.NECK_MAPS + [M.NECK_APART])
def test_neck_emulation_inside_bounds(shape):
    cases, terms = neck_set(shape)
    for b in range(3):
        for mode in ("fp32",) + MIXED:
            dw, dx = M.neck_emulate(*cases[b], mode)
            rw, rx, bw, bx = M.neck_grad_bounds_mixed(*cases[b], mode, terms=terms[b])
            fw, fx = M.worst(dw, rw, bw)[0], M.worst(dx, rx, bx)[0]
            print(f"neck {shape} branch {b} {mode}: emulation at {fw:.3f} (dw), {fx:.3f} (dx) of the bound")
            assert fw <= 1.0 and fx <= 1.0, (shape, b, mode, fw, fx)


def test_mixed_bounds_contain_the_plain_ones():
    case, t = down_set(M.DOWN_SHAPES[0])
    for mode in MIXED:
        _, _, bw, bx, _ = M.down_grad_bounds_mixed(*case, mode, terms=t)
        assert (bw > t["bw"]).all() and (bx >= t["bx"]).all()
    _, _, bw, bx, ties = M.down_grad_bounds_mixed(*case, "fp32", terms=t)
    assert bw is t["bw"] and bx is t["bx"] and ties is t["ties"]


def test_matrix_form_of_the_wgrad_is_the_reference_s():
    x, w, z, dy = M.down_case(64, 64, 7, 5, 2, seed=9)
    dz = M.D.norm_backward(z, dy)
    a, b = M.wgrad_s2(dz, x.astype(np.float64)), M.D.conv_s2_wgrad(dz, x.astype(np.float64))
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


def test_down_bound_flags_near_ties():
    x, w, z, dy = M.down_case(64, 64, 6, 6, 1, seed=5)
    z = z.copy()
    xhat = M.D.norm(z.astype(np.float64))[0]
    i = np.unravel_index(np.abs(xhat).argmin(), xhat.shape)
    mean = z[i[0], i[1]].astype(np.float64).mean()
    z[i] = np.float32(mean)  # xhat of this element ~ 0 (the plane's mean moves by 1 / 9 of the change)
    *_, ties = M.down_grad_bounds_mixed(x, w, z, dy, "bf16", tie=0.2)
    assert ties[i]


def told_apart(rw, bw_plain, emul):
    """bf16 leaves the plain fp32 bound at its worst element; bf16x3's largest deviation is under 1 / 16 of bf16's."""
    d16 = np.abs(emul["bf16"] - rw)
    d3 = np.abs(emul["bf16x3"] - rw)
    return float((d16 / bw_plain).max()), float(d3.max() / d16.max())


def test_down_modes_are_told_apart():
    case, t = down_set(M.DOWN_APART)
    frac, ratio = told_apart(t["dw"], t["bw"], {m: M.down_emulate(*case, m)[0] for m in MIXED})
    print(f"down: bf16 dw at {frac:.1f} x the fp32 bound, bf16x3 / bf16 deviation {ratio:.4f}")
    assert frac > 1.0 and ratio < 1.0 / 16


def test_neck_modes_are_told_apart():
    cases, terms = neck_set(M.NECK_APART)
    b = M.NECK_APART_BRANCH
    frac, ratio = told_apart(terms[b]["dw"], terms[b]["bw"], {m: M.neck_emulate(*cases[b], m)[0] for m in MIXED})
    print(f"neck: bf16 dw at {frac:.1f} x the fp32 bound, bf16x3 / bf16 deviation {ratio:.4f}")
    assert frac > 1.0 and ratio < 1.0 / 16
