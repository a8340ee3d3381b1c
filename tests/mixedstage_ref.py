"""CPU side of the mixed-precision strided-stage and upsampler backwards (pp_down_backward_mp, csrc/down_train16.hip;
pp_neck_backward_mp, csrc/neck_train16.hip): an emulation of the modes' arithmetic and the element-wise a-priori bounds that
downtrain_ref.grad_bounds and necktrain_ref.grad_bounds become when the operands of the two gradient products are 16-bit.  Both
reference modules and mixedtrain_ref (bf16_round, bf16_split, MODES, U16, TINY) are imported and left as they are.

Modes, as for the units (mixedtrain_ref).  In both families everything up to dz (the statistics, the mask, the norm backward) is the
fp32 path's, so the kernels round or split the fp32 dz, the fp32 inputs x and w, and nothing else:
  "bf16":    every operand rounded once (round to nearest even): a product of two rounded operands carries eps = 2 u16 + u16^2;  m = 1
  "bf16x3":  x = hi + lo, hi = bf16(x), lo = bf16(fl32(x - hi)), a product is hi hi + hi lo + lo hi: eps = 3 u16^2;             m = 3

Bounds, U = 2^-24, in the form DESIGN.md states for the units.  With bw, bx the family's own fp32 bounds and K the length of the sum:
  bw_mixed = bw + 1.01 (eps sum |dz operand| + (m - 1) K U sum |dz operand|)           K = nb x positions
  bx_mixed = bx + 1.01 (eps + (m - 1) K U) sum |w| |dz|                                K = 4 Cout (down), Cup s s (neck)
The m MFMAs of a product add (m - 1) K terms to the fp32 accumulation, whatever their order.  The operand error is relative to the
fp32 dz, which lies within the family's e_dz (down) or E (neck) of the exact one.  Down: eps sum e_dz |x| is below the 1 % by which
downtrain_ref.grad_bounds inflates its own sum e_dz |x| term (eps < 2^-7 < 0.01).  Neck: necktrain_ref.grad_bounds has no such
inflation, so eps sum |x| E (the bound's ew term, recovered as bw - sum_bound) is added explicitly.  A lo part in the subnormal range
may be flushed by the MFMA: bf16x3 carries 2^-126 sum |other operand|, bounded by the term count times the largest magnitude.  The
mask is fp32's, so the down bound flags near-ties exactly as downtrain_ref.grad_bounds does (its jumps are part of bw, bx)."""
import numpy as np

import downtrain_ref as D
import necktrain_ref as N
from mixedtrain_ref import MODES, TINY, U16, U32, bf16_round, bf16_split  # noqa: F401

# the cases of tests/test_mixedstage_gpu.py, cleared by tests/test_mixedstage_cpu.py
DOWN_SHAPES = [(64, 64, 33, 18, 1), (64, 128, 40, 26, 2), (128, 256, 25, 9, 3), (128, 256, 2, 3, 2), (64, 128, 1, 4, 1),
               (64, 64, 260, 254, 1)]  # (cin, cout, hin, win, nb); the last: 130 x 127 output plane, two plane segments, odd pitch
NECK_MAPS = [(40, 24, 3), (20, 36, 1), (4, 4, 2)]  # (H, W, nb) of the level-0 map; (4, 4): level 2 is one input pixel
DOWN_APART = (64, 64, 20, 18, 1)  # "the modes are told apart": 10 x 9 = 90 output positions, one frame
NECK_APART = (4, 4, 1)            # branch NECK_APART_BRANCH on a 4 x 4 map, one frame: the plain neck bound grows with the pixel count
NECK_APART_BRANCH = 1             # faster than bf16's error does, and a 12 x 8 map no longer leaves it (tests/test_mixedstage_cpu.py)
_f64 = lambda t: np.asarray(t, np.float64)  # noqa: E731


def down_case(cin, cout, hin, win, nb, seed=None):
    """x, w, z (the float32 conv output, moved off the ReLU's zero by blocktrain_ref.tie_free), dy: test_downtrain_gpu.random_case."""
    rng = np.random.default_rng(100 + cout + hin if seed is None else seed)
    x = rng.standard_normal((nb, cin, hin, win)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 3, 3)) * 0.05).astype(np.float32)
    z = D.tie_free(D.conv_s2(x.astype(np.float64), w.astype(np.float64)))
    dy = rng.standard_normal(z.shape).astype(np.float32)
    return x, w, z, dy


def neck_case(H, W, nb, seed=None):
    """xs, ws (per branch), y [nb, 320, H, W] (the float32 cast of the float64 forward), dy: test_necktrain_gpu.random_case."""
    rng = np.random.default_rng(100 + H if seed is None else seed)
    xs = [rng.standard_normal((nb, N.CIN[b], H >> b, W >> b)).astype(np.float32) for b in range(3)]
    ws = [(rng.standard_normal((N.CIN[b], N.CUP[b], 1 << b, 1 << b)) * 0.05).astype(np.float32) for b in range(3)]
    y = np.concatenate([N.branch_forward(xs[b], ws[b]) for b in range(3)], 1).astype(np.float32)
    dy = rng.standard_normal((nb, 320, H, W)).astype(np.float32)
    return xs, ws, y, dy


def branch_slice(b):
    return slice(N.COFF[b], N.COFF[b] + N.CUP[b])


def _product(f, a, b, mode):
    """The bilinear f(a, b) in float64 with float32 operands a, b taken as the mode takes them ("fp32": as they are)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if mode == "fp32":
        return f(_f64(a), _f64(b))
    if mode == "bf16":
        return f(_f64(bf16_round(a)), _f64(bf16_round(b)))
    if mode == "bf16x3":
        (ah, al), (bh, bl) = ((_f64(p) for p in bf16_split(t)) for t in (a, b))
        return f(ah, bh) + f(ah, bl) + f(al, bh)
    raise ValueError(mode)


# ------------------------------------------------------------------ the strided stage
def wgrad_s2(dz, x):
    """downtrain_ref.conv_s2_wgrad as one matrix product per tap and frame (the same sums; its einsum form takes seconds on the
    16 510-element planes of the largest case)."""
    nb, co = dz.shape[:2]
    zr = np.ascontiguousarray(dz, np.float64).reshape(nb, co, -1)
    dw = np.empty((co, x.shape[1], 3, 3))
    for ky in range(3):
        for kx in range(3):
            v = np.ascontiguousarray(D.tap_view(x, ky, kx), np.float64).reshape(nb, x.shape[1], -1)
            dw[:, :, ky, kx] = sum(zr[f] @ v[f].T for f in range(nb))
    return dw


def down_emulate(x, w, z, dy, mode):
    """The arithmetic of a mode without its fp32 accumulation: dz in float64 rounded once to float32 (what every mode's norm backward
    stores), the operands of the two products rounded or split, products and sums in float64 -> dw, dx."""
    hin, win = np.shape(x)[-2:]
    dz32 = D.norm_backward(z, dy).astype(np.float32)
    dw = _product(wgrad_s2, dz32, x, mode)
    dx = _product(lambda a, b: D.conv_s2_dgrad(a, b, hin, win), dz32, w, mode)
    return dw, dx


def down_terms(x, w, z, dy, tie=1e-5):
    """downtrain_ref.grad_bounds and the two sums of absolute products the mixed bounds add to it (mode-independent)."""
    dw, dx, bw, bx, ties = D.grad_bounds(x, w, z, dy, tie)
    hin, win = np.shape(x)[-2:]
    adz, ax_, aw_ = np.abs(D.norm_backward(z, dy)), np.abs(_f64(x)), np.abs(_f64(w))
    nb, cout, ho, wo = adz.shape
    return dict(dw=dw, dx=dx, bw=bw, bx=bx, ties=ties, aw=wgrad_s2(adz, ax_), ax=D.conv_s2_dgrad(adz, aw_, hin, win),
                Kw=nb * ho * wo, Kx=4 * cout, zmax=float(adz.max()), xmax=float(ax_.max()), wmax=float(aw_.max()))


def _mixed(t, mode, extra_w=0.0, extra_x=0.0):
    if mode == "fp32":
        return t["bw"], t["bx"]
    eps, m = MODES[mode]
    bw = t["bw"] + 1.01 * (eps * (t["aw"] + extra_w) + (m - 1) * t["Kw"] * U32 * t["aw"])
    bx = t["bx"] + 1.01 * (eps * (t["ax"] + extra_x) + (m - 1) * t["Kx"] * U32 * t["ax"])
    if m == 3:
        bw = bw + 1.01 * TINY * t["Kw"] * (t["zmax"] + t["xmax"])
        bx = bx + 1.01 * TINY * t["Kx"] * (t["zmax"] + t["wmax"])
    return bw, bx


def down_grad_bounds_mixed(x, w, z, dy, mode, tie=1e-5, terms=None):
    """-> dw, dx (float64, exact inputs), the element-wise bounds of a mode's deviation from them, and the near-tie set."""
    t = down_terms(x, w, z, dy, tie) if terms is None else terms
    bw, bx = _mixed(t, mode)
    return t["dw"], t["dx"], bw, bx, t["ties"]


# ------------------------------------------------------------------ the upsampling branch
def neck_dz(x, w, y, dy):
    """dZ of necktrain_ref.branch_backward in the GEMM layout [nb, R, p], float64."""
    x64, w64 = _f64(x), _f64(w)
    s = w64.shape[2]
    Z = N.conv_t(x64, w64)
    mean, rstd = N.norm_stats(Z)
    xhat = (Z - mean) * rstd
    Gr = _f64(dy) * (np.asarray(y) > 0)
    return N.to_rows(rstd * (Gr - Gr.mean((2, 3), keepdims=True) - xhat * (Gr * xhat).mean((2, 3), keepdims=True)), s)


def neck_emulate(x, w, y, dy, mode):
    """As down_emulate: dZ rounded once to float32, the operands of dw = sum x dZ and dx = sum w dZ as the mode takes them."""
    nb, cin = np.shape(x)[:2]
    dz32 = neck_dz(x, w, y, dy).astype(np.float32)
    X, Wr = np.asarray(x, np.float32).reshape(nb, cin, -1), np.asarray(w, np.float32).reshape(cin, -1)
    dw = _product(lambda a, b: np.matmul(b, a.transpose(0, 2, 1)).sum(0), dz32, X, mode).reshape(np.shape(w))
    dx = _product(lambda a, b: np.matmul(b[None], a), dz32, Wr, mode).reshape(np.shape(x))
    return dw, dx


def neck_terms(x, w, y, dy):
    dw, dx, bw, bx = N.grad_bounds(x, w, y, dy)
    _, _, (aw, ax), _ = N.branch_backward(x, w, y, dy, bounds=True)
    nb, cin, h, wd = np.shape(x)
    R = int(np.prod(np.shape(w)[1:]))
    Kw, Kx = nb * h * wd, R
    ew, ex = bw - N.sum_bound(Kw, aw, dw), bx - N.sum_bound(Kx, ax, dx)  # sum |x| E, sum |w| E of necktrain_ref.grad_bounds
    return dict(dw=dw, dx=dx, bw=bw, bx=bx, aw=aw, ax=ax, ew=np.maximum(ew, 0.0), ex=np.maximum(ex, 0.0), Kw=Kw, Kx=Kx,
                zmax=float(np.abs(neck_dz(x, w, y, dy)).max()), xmax=float(np.abs(x).max()), wmax=float(np.abs(w).max()))


def neck_grad_bounds_mixed(x, w, y, dy, mode, terms=None):
    """-> dw, dx (float64, exact inputs) and the element-wise bounds of a mode's deviation from them."""
    t = neck_terms(x, w, y, dy) if terms is None else terms
    bw, bx = _mixed(t, mode, t["ew"], t["ex"])
    return t["dw"], t["dx"], bw, bx


def worst(got, want, bound):
    """The largest fraction of the bound and the largest deviation."""
    dev = np.abs(_f64(got) - want)
    return float((dev / bound).max()), float(dev.max())
