"""CPU side of the mixed-precision Resnet unit backward (pp_unit_backward_mp, csrc/block_train16.hip): bf16 rounding and splitting in
numpy, an emulation of the two modes' arithmetic, and the element-wise a-priori bounds that blocktrain_ref.grad_bounds becomes when
the operands of the two gradient products are 16-bit.  blocktrain_ref is imported and left as it is.

Modes.  "bf16": every operand of the wgrad and dgrad products is rounded once to bf16 (round to nearest even), products and sums in
fp32.  "bf16x3": every operand is split x = hi + lo, hi = bf16(x), lo = bf16(fl32(x - hi)), and a product is hi hi + hi lo + lo hi.
Everything else (statistics, a = relu(xhat) in fp32, mask, norm backward, the reduction of dw) is the fp32 implementation's.

Bounds, u16 = 2^-8 the bf16 rounding unit, U = 2^-24:
  bf16:    a product of two rounded operands carries the relative error eps = 2 u16 + u16^2;                       m = 1 MFMA
  bf16x3:  x = hi + lo + e with |e| <= u16^2 |x|, the dropped lo lo term is at most u16^2 |a b|: eps = 3 u16^2;    m = 3 MFMAs,
           which triple the fp32 accumulation term
  bw_mixed  = bw  + 1.01 (eps sum|dz a| + (m - 1) nb N U sum|dz a|)
  eda_mixed = eda + 1.01 (eps + (m - 1) 9 C U) conv3_dgrad(|dz|, |w|), pushed through grad_bounds' own norm-backward propagation
              (eGr -> ec1, ec2 -> bu), restated below term by term; near-ties are handled as there, because the mask is fp32's.
A lo part in the subnormal range may be flushed by the MFMA; bf16x3 therefore carries the absolute term 2^-126 sum|other operand|,
which is invisible at any magnitude a test uses and makes the bound hold either way.

grad_bounds' terms are restated here (with its convolution sums as matrix products, so that the 16 510-element planes of the GPU tests
cost a fraction of a second) and evaluated once per input set; tests/test_mixedtrain_cpu.py asserts that the restatement with no
operand error is blocktrain_ref.grad_bounds."""
import numpy as np

import blocktrain_ref as B

U16 = 2.0 ** -8
U32 = B.U32
MODES = {"bf16": (2 * U16 + U16 * U16, 1), "bf16x3": (3 * U16 * U16, 3)}  # eps per product, MFMAs per product
TINY = 2.0 ** -126


def bf16_round(x):
    """float32 -> the nearest bf16 (ties to even), returned as float32.  Finite inputs."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def bf16_split(x):
    """-> hi, lo (float32 holding bf16 values): hi = bf16(x), lo = bf16(fl32(x - hi))."""
    x = np.ascontiguousarray(x, np.float32)
    hi = bf16_round(x)
    return hi, bf16_round((x - hi).astype(np.float32))


def a_fp32(u):
    """xhat and a = relu(xhat) as k_unit_pack evaluates them: mean and rstd from float64 sums, rounded to float32, then
    fl(fl(u - mean) rstd) in float32."""
    u32 = np.asarray(u, np.float32)
    u64 = u32.astype(np.float64)
    n = u64.shape[2] * u64.shape[3]
    mean = u64.sum((2, 3), keepdims=True) / n
    var = np.maximum((u64 * u64).sum((2, 3), keepdims=True) / n - mean * mean, 0.0)
    meanf, rstdf = mean.astype(np.float32), (1.0 / np.sqrt(var + B.EPS)).astype(np.float32)
    xhat = ((u32 - meanf).astype(np.float32) * rstdf).astype(np.float32)
    return xhat, np.maximum(xhat, np.float32(0)), rstdf


def emulate(u, w, dz, mode, dskip=None):
    """The arithmetic of a mode without its fp32 accumulation: operands rounded (bf16) or split (bf16x3), products and sums in float64,
    a evaluated in float32, the mask that of the float32 xhat, the norm backward in float64 -> dw, du."""
    xhat, a, rstd = a_fp32(u)
    w32, dz32 = np.asarray(w, np.float32), np.asarray(dz, np.float32)
    f64 = lambda t: t.astype(np.float64)  # noqa: E731
    if mode == "bf16":
        ah, wh, zh = (f64(bf16_round(t)) for t in (a, w32, dz32))
        dw, da = B.conv3_wgrad(zh, ah), B.conv3_dgrad(zh, wh)
    elif mode == "bf16x3":
        (ah, al), (wh, wl), (zh, zl) = ((f64(p) for p in bf16_split(t)) for t in (a, w32, dz32))
        dw = B.conv3_wgrad(zh, ah) + B.conv3_wgrad(zh, al) + B.conv3_wgrad(zl, ah)
        da = B.conv3_dgrad(zh, wh) + B.conv3_dgrad(zl, wh) + B.conv3_dgrad(zh, wl)
    else:
        raise ValueError(mode)
    x64, r64 = f64(xhat), f64(rstd)
    Gr = da * (xhat > 0)
    du = r64 * (Gr - Gr.mean((2, 3), keepdims=True) - x64 * (Gr * x64).mean((2, 3), keepdims=True))
    if dskip is not None:
        du = du + np.asarray(dskip, np.float64)
    return dw, du


def wgrad(dz, a):
    """blocktrain_ref.conv3_wgrad as one matrix product per tap and frame (the same sums; the large planes of the GPU tests take
    seconds in the einsum form)."""
    nb, C = dz.shape[:2]
    z = np.ascontiguousarray(dz, np.float64).reshape(nb, C, -1)
    a = np.broadcast_to(a, (nb,) + a.shape[1:]) if a.shape[0] != nb else a
    dw = np.empty((C, a.shape[1], 3, 3))
    for ky in range(3):
        for kx in range(3):
            s = np.ascontiguousarray(B.shifted(a, ky - 1, kx - 1), np.float64).reshape(nb, a.shape[1], -1)
            dw[:, :, ky, kx] = sum(z[f] @ s[f].T for f in range(nb))
    return dw


_LAST = None  # the inputs (kept alive, compared by identity: do not modify them in place between calls) and the terms of the last
              # evaluation, so that the dskip variant of a case costs nothing


def _terms(u, w, dz, tie):
    """What the bounds are made of and dskip does not touch, named as in blocktrain_ref.grad_bounds."""
    global _LAST
    if _LAST is not None and _LAST[0] is u and _LAST[1] is w and _LAST[2] is dz and _LAST[3] == tie:
        return _LAST[4]
    u64, w64, dz64 = np.asarray(u, np.float64), np.asarray(w, np.float64), np.asarray(dz, np.float64)
    xhat, mean, rstd = B.norm(u64)
    a = np.maximum(xhat, 0.0)
    xmax = np.abs(xhat).max((2, 3), keepdims=True)
    ex = U32 * (rstd * np.abs(mean) + 4.0 * np.maximum(1.0, xmax))
    adz, aw64 = np.abs(dz64), np.abs(w64)
    t = dict(xhat=xhat, rstd=rstd, a=a, ex=ex, dw=wgrad(dz64, a), aw=wgrad(adz, a), exw=wgrad(adz, np.broadcast_to(ex, a.shape)),
             da=B.conv3_dgrad(dz64, w64), awz=B.conv3_dgrad(adz, aw64), ties=np.abs(xhat) < tie,
             zmax=float(adz.max()), amax=float(a.max()), wmax=float(aw64.max()))
    _LAST = (u, w, dz, tie, t)
    return t


def _bounds(u, w, dz, dskip, tie, eps, m):
    """blocktrain_ref.grad_bounds, term by term, with the relative operand error eps per product and m MFMAs per product; eps = 0,
    m = 1 is grad_bounds itself (tests/test_mixedtrain_cpu.py holds the two together)."""
    t = _terms(u, w, dz, tie)
    nb, C, h, wd = np.shape(u)
    N = h * wd
    xhat, rstd, ex, dw, aw, da, awz, ties = (t[k] for k in ("xhat", "rstd", "ex", "dw", "aw", "da", "awz", "ties"))
    mask = t["a"] > 0
    bw = 1.01 * (nb * N * U32 * aw + t["exw"] + U32 * np.abs(dw) + 1e-45) + 1.01 * (eps * aw + (m - 1) * nb * N * U32 * aw)
    eda = 9 * C * U32 * awz + U32 * np.abs(da) + 1.01 * (eps + (m - 1) * 9 * C * U32) * awz
    if m == 3:  # lo parts the MFMA may flush: 2^-126 sum |other operand|, the sums bounded by term count x largest magnitude
        bw = bw + 1.01 * TINY * nb * N * (t["zmax"] + t["amax"])
        eda = eda + 1.01 * TINY * 9 * C * (t["zmax"] + t["wmax"])
    Gr, eGr = da * mask, eda * mask
    c1 = Gr.mean((2, 3), keepdims=True)
    c2 = (Gr * xhat).mean((2, 3), keepdims=True)
    ec1 = eGr.mean((2, 3), keepdims=True) + U32 * np.abs(c1)
    ec2 = (eGr * np.abs(xhat) + np.abs(Gr) * ex).mean((2, 3), keepdims=True) + U32 * np.abs(c2)
    t3 = Gr - c1 - xhat * c2
    du0 = rstd * t3
    du = du0 if dskip is None else du0 + np.asarray(dskip, np.float64)
    bu = rstd * (eGr + ec1 + ex * np.abs(c2) + np.abs(xhat) * ec2 + U32 * (np.abs(Gr - c1) + np.abs(xhat * c2) + np.abs(t3))) \
        + 2 * U32 * np.abs(du0) + U32 * np.abs(du) + 1e-45
    if ties.any():
        for f, c, y, x in zip(*np.nonzero(ties)):
            jump = rstd[f, c, 0, 0] * abs(da[f, c, y, x])
            bu[f, c] += jump * (1.0 + np.abs(xhat[f, c] * xhat[f, c, y, x])) / N
            bu[f, c, y, x] += jump
    return dw, du, bw, 1.01 * bu, ties


def grad_bounds_mixed(u, w, dz, mode, dskip=None, tie=1e-5):
    """-> dw, du (float64, exact inputs), the element-wise bounds bw_mixed, bu_mixed of a mode's deviation from them, and the near-tie
    set: blocktrain_ref.grad_bounds with the two product terms widened as the module docstring derives."""
    eps, m = MODES[mode]
    return _bounds(u, w, dz, dskip, tie, eps, m)
