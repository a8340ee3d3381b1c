"""CPU restatement (numpy, float64) of training the BatchNorm RPN with batch statistics: every BatchNorm2d(eps 1e-3) in train mode
normalises a channel with mean = sum v / N and the biased var = sum v^2 / N - mean^2 over the N = nb h w elements of all frames, and is
then the affine norm(v) = scale v + shift, scale = gamma / sqrt(var + 1e-3), shift = beta - mean scale.  The three backward primitives
(csrc/block_train.hip, down_train.hip, neck_train.hip: pp_*_backward_bn), the forward and the whole chain, wired by the table of
rpntrain_ref.  Pinned to the reference's own autograd by tests/golden/bnbatch_small.npz (tests/test_bnbatch_cpu.py); the GPU tests use
it where no golden can be stored.

With g the gradient behind the ReLU, v the norm's input, r = 1 / sqrt(var + 1e-3), dshift = sum g, dscale = sum g v (all frames):
    c1 = dshift / N,  c2 = r (dscale - mean dshift) / N,  vhat = (v - mean) r,  dv = scale ((g - c1) - vhat c2)
and dgamma = r (dscale - mean dshift) = sum g vhat, dbeta = dshift (bntrain_ref.affine_grad with the batch statistics).

The primitives take scale, shift, mean, var as GIVEN values (the library's are float32), so fma(v, scale, shift) is rounded once and keeps
the sign of the exact value: the ReLU mask of a float32 evaluation IS the float64 mask, no near-ties.  The a-priori bounds (`*_bounds`)
are for a float32 implementation working from the same inputs, U = 2^-24, first order, inflated by 1 %, float32 summation in any
order; the pooled sums and c1, c2 are formed in float64 and rounded once."""
import numpy as np

import blocktrain_ref as B
import bntrain_ref as A
import downtrain_ref as D
import necktrain_ref as N
from bntrain_ref import BN_PREFIXES, EPS, LAYER_KEYS, PARAM_KEYS, U32, U64, aff, bn_prefix, ch, sums  # noqa: F401
from rpntrain_ref import CONV_KEYS, NECK_KEYS, RPN_TABLE, W0

MOMENTUM = 0.01  # the reference's BatchNorm2d(eps=1e-3, momentum=0.01)


def batch_stats(v):
    """-> mean, biased var per channel of v [nb,C,h,w], float64."""
    v = np.asarray(v, np.float64)
    return v.mean((0, 2, 3)), v.var((0, 2, 3))


def stats32(v):
    """The statistics as the library rounds them: float64 sums, each value rounded once to float32."""
    m, s = batch_stats(v)
    return m.astype(np.float32), s.astype(np.float32)


def fold(gamma, beta, mean, var):
    return A.fold(gamma, beta, mean, var)


fold32 = A.fold32
affine_grad = A.affine_grad


def moved(running_mean, running_var, mean, var, n):
    """BatchNorm2d's update of the running statistics after one forward over n elements per channel (unbiased variance), float64."""
    rm, rv = np.asarray(running_mean, np.float64), np.asarray(running_var, np.float64)
    return (1.0 - MOMENTUM) * rm + MOMENTUM * np.asarray(mean, np.float64), (1.0 - MOMENTUM) * rv + MOMENTUM * (n / (n - 1.0)) * np.asarray(var, np.float64)


def norm_backward(g, v, scale, mean, var):
    """g, v [nb,C,h,w] -> dv, dscale, dshift, and (c1, c2, vhat, r) for the bounds."""
    n = g.shape[0] * g.shape[2] * g.shape[3]
    r = 1.0 / np.sqrt(np.asarray(var, np.float64) + EPS)
    ds, dh = sums(g, v)
    c1, c2 = dh / n, r * (ds - np.asarray(mean, np.float64) * dh) / n
    vhat = (v - ch(mean)) * ch(r)
    return ch(scale) * ((g - ch(c1)) - vhat * ch(c2)), ds, dh, (c1, c2, vhat, r)


def norm_backward_bound(g, eg, v, ev, scale, mean, var, bs, bh):
    """The bound of |dv32 - dv| for dv32 = fl(scale fl(fl(g32 - c1_32) - fl(vhat32 c2_32))): |g32 - g| <= eg, |v32 - v| <= ev element-wise,
    the pooled sums off by bs, bh per channel.  c1, c2: float64 expressions of the sums, rounded once; r32 = fl(r); vhat32 = fl(fl(v32 -
    mean) r32), three roundings of a quantity of size |vhat| and ev r."""
    n = g.shape[0] * g.shape[2] * g.shape[3]
    dv, ds, dh, (c1, c2, vhat, r) = norm_backward(g, v, scale, mean, var)
    am = np.abs(np.asarray(mean, np.float64))
    e1 = bh / n + U32 * np.abs(c1)
    e2 = r * (bs + am * bh) / n + 8 * U64 * r * (np.abs(ds) + am * np.abs(dh)) / n + U32 * np.abs(c2)
    evh = ev * ch(r) + 3 * U32 * np.abs(vhat)
    t = vhat * ch(c2)
    et = np.abs(vhat) * ch(e2) + evh * np.abs(ch(c2)) + U32 * np.abs(t)
    s1 = g - ch(c1)
    es = eg + ch(e1) + U32 * np.abs(s1) + et + U32 * np.abs(s1 - t)
    return np.abs(ch(scale)) * es + U32 * np.abs(dv)


# ------------------------------------------------------------------ unit: BatchNorm (batch statistics) -> ReLU -> Conv3x3
unit_forward = A.unit_forward


def unit_backward(u, w, scale, shift, mean, var, dz, dskip=None):
    """-> dw, du, dscale = sum g u, dshift = sum g (float64)."""
    u64, w64, dz64 = (np.asarray(t, np.float64) for t in (u, w, dz))
    a = np.maximum(aff(u64, scale, shift), 0.0)
    g = B.conv3_dgrad(dz64, w64) * (a > 0)
    du, ds, dh, _ = norm_backward(g, u64, scale, mean, var)
    if dskip is not None:
        du = du + np.asarray(dskip, np.float64)
    return B.conv3_wgrad(dz64, a), du, ds, dh


def unit_bounds(u, w, scale, shift, mean, var, dz, dskip=None):
    """-> (dw, du, dscale, dshift), (bw, bu, bs, bh).  dw, the dgrad product da and the two sums as bntrain_ref.unit_bounds; du by
    norm_backward_bound (+ dskip, one more rounding)."""
    u64, w64, dz64 = (np.asarray(t, np.float64) for t in (u, w, dz))
    nb, C, h, wd = u64.shape
    out = unit_backward(u, w, scale, shift, mean, var, dz, dskip)
    a = np.maximum(aff(u64, scale, shift), 0.0)
    mask = a > 0
    bw = (nb * h * wd + 1) * U32 * B.conv3_wgrad(np.abs(dz64), a) + U32 * np.abs(out[0]) + 1e-45
    da = B.conv3_dgrad(dz64, w64)
    eg = (9 * C * U32 * B.conv3_dgrad(np.abs(dz64), np.abs(w64)) + U32 * np.abs(da)) * mask
    g = da * mask
    n = nb * h * wd
    bs = (eg * np.abs(u64)).sum((0, 2, 3)) + n * U64 * (np.abs(g * u64)).sum((0, 2, 3)) + 1e-300
    bh = eg.sum((0, 2, 3)) + n * U64 * np.abs(g).sum((0, 2, 3)) + 1e-300
    bu = norm_backward_bound(g, eg, u64, 0.0, scale, mean, var, bs, bh) + (U32 * np.abs(out[1]) if dskip is not None else 0.0) + 1e-45
    return out, tuple(1.01 * b for b in (bw, bu, bs, bh))


# ------------------------------------------------------------------ stage: Conv3x3 stride 2 -> BatchNorm (batch statistics) -> ReLU
down_forward = A.down_forward


def down_backward(x, w, z, scale, shift, mean, var, dy):
    """-> dw, dx, dscale = sum g z, dshift = sum g (float64); z is the conv output the forward stored."""
    x64, w64, z64 = (np.asarray(t, np.float64) for t in (x, w, z))
    g = np.asarray(dy, np.float64) * (aff(z64, scale, shift) > 0)
    dz, ds, dh, _ = norm_backward(g, z64, scale, mean, var)
    return D.conv_s2_wgrad(dz, x64), D.conv_s2_dgrad(dz, w64, *x64.shape[-2:]), ds, dh


def down_bounds(x, w, z, scale, shift, mean, var, dy):
    """g = dy [mask] is exact and the sums are float64 sums of exact products; dz32 is off by edz (norm_backward_bound), which the two
    products carry on top of their own summation error (K_w = nb ho wo, K_x <= 4 Cout)."""
    x64, w64, z64 = (np.asarray(t, np.float64) for t in (x, w, z))
    nb, cout, ho, wo = z64.shape
    hin, win = x64.shape[-2:]
    out = down_backward(x, w, z, scale, shift, mean, var, dy)
    g = np.asarray(dy, np.float64) * (aff(z64, scale, shift) > 0)
    n = nb * ho * wo
    bs = n * U64 * np.abs(g * z64).sum((0, 2, 3)) + 1e-300
    bh = n * U64 * np.abs(g).sum((0, 2, 3)) + 1e-300
    dz = norm_backward(g, z64, scale, mean, var)[0]
    edz = norm_backward_bound(g, 0.0, z64, 0.0, scale, mean, var, bs, bh)
    bw = (n + 1) * U32 * D.conv_s2_wgrad(np.abs(dz), np.abs(x64)) + D.conv_s2_wgrad(edz, np.abs(x64)) + U32 * np.abs(out[0]) + 1e-45
    bx = (4 * cout + 1) * U32 * D.conv_s2_dgrad(np.abs(dz), np.abs(w64), hin, win) + D.conv_s2_dgrad(edz, np.abs(w64), hin, win) \
        + U32 * np.abs(out[1]) + 1e-45
    return out, tuple(1.01 * b for b in (bw, bx, bs, bh))


# ------------------------------------------------------------------ branch: ConvTranspose(k = s) -> BatchNorm (batch statistics) -> ReLU
branch_forward = A.branch_forward


def branch_backward(x, w, scale, mean, var, y, dy, bounds=False):
    """y / dy: the branch's channel slice of rpn_out and of its gradient; the mask is the GIVEN y -> dw, dx, dscale = sum g Z,
    dshift = sum g (float64).  bounds=True: and their a-priori bounds.  Z32 is a float32 sum of Cin products, |Z32 - Z| <= eZ = (Cin + 1)
    U sum |w x|; g is exact; dZ32 by norm_backward_bound; dw sums K_w = nb h w products, dx K_x = Cup s s."""
    x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    nb, cin, h, wd = x64.shape
    s = w64.shape[2]
    Z = N.conv_t(x64, w64)
    g = np.asarray(dy, np.float64) * (np.asarray(y) > 0)
    dZ, ds, dh, _ = norm_backward(g, Z, scale, mean, var)
    dZr = N.to_rows(dZ, s)
    X, Wr = x64.reshape(nb, cin, -1), w64.reshape(cin, -1)
    dw = np.matmul(X, dZr.transpose(0, 2, 1)).sum(0).reshape(w64.shape)
    dx = np.matmul(Wr[None], dZr).reshape(x64.shape)
    out = (dw, dx, ds, dh)
    if not bounds:
        return out
    eZ = (cin + 1) * U32 * N.conv_t(np.abs(x64), np.abs(w64))
    n = nb * Z.shape[2] * Z.shape[3]
    bs = (np.abs(g) * eZ).sum((0, 2, 3)) + n * U64 * np.abs(g * Z).sum((0, 2, 3)) + 1e-300
    bh = n * U64 * np.abs(g).sum((0, 2, 3)) + 1e-300
    edZr = N.to_rows(norm_backward_bound(g, 0.0, Z, eZ, scale, mean, var, bs, bh), s)
    aw = np.matmul(np.abs(X), np.abs(dZr).transpose(0, 2, 1)).sum(0).reshape(w64.shape)
    ax = np.matmul(np.abs(Wr)[None], np.abs(dZr)).reshape(x64.shape)
    bw = (nb * h * wd + 1) * U32 * aw + np.matmul(np.abs(X), edZr.transpose(0, 2, 1)).sum(0).reshape(w64.shape) + U32 * np.abs(dw) + 1e-45
    bx = (w64.shape[1] * s * s + 1) * U32 * ax + np.matmul(np.abs(Wr)[None], edZr).reshape(x64.shape) + U32 * np.abs(dx) + 1e-45
    return out, tuple(1.01 * b for b in (bw, bx, bs, bh))


# ------------------------------------------------------------------ the whole RPN
def rpn_forward(canvas, wc, wn, bn):
    """canvas [nb,64,gx,gy], wc the sixteen convolutions in CONV_KEYS order, wn the three upsamplers, bn {BatchNorm prefix: (gamma,
    beta, ...)} -> dict: y, taps, units, zs as rpntrain_ref.rpn_forward, stats {prefix: (mean, biased var, n)} and folds {prefix:
    (scale, shift)}, all float64 (nothing is rounded on the way)."""
    stats, folds = {}, {}
    x = np.asarray(canvas, np.float64)

    def norm(v, key):
        p = bn_prefix(key)
        m, s = batch_stats(v)
        stats[p] = (m, s, v.shape[0] * v.shape[2] * v.shape[3])
        folds[p] = fold(bn[p][0], bn[p][1], m, s)
        return np.maximum(aff(v, *folds[p]), 0.0)

    taps, units, zs, ys = [], [], [], []
    for b, mods in RPN_TABLE:
        keys = CONV_KEYS[W0[b]:W0[b] + 1 + sum(mods)]
        w = [np.asarray(t, np.float64) for t in wc[W0[b]:W0[b] + 1 + sum(mods)]]
        U = lambda r, i: B.conv3(norm(r, keys[i]), w[i])  # noqa: E731
        z = D.conv_s2(x, w[0])
        r = norm(z, keys[0])
        us, i = [], 1
        for n in mods:
            us.append(r)
            if n == 2:
                us.append(U(r, i))
                r = r + U(us[-1], i + 1)
            else:
                r = r + U(r, i)
            i += n
        x = r
        taps.append(x), units.append(us), zs.append(z)
        ys.append(norm(N.conv_t(x, np.asarray(wn[b], np.float64)), NECK_KEYS[b]))
    return dict(y=np.concatenate(ys, 1), taps=taps, units=units, zs=zs, stats=stats, folds=folds)


def relu_masks(fwd):
    return A.relu_masks(fwd["y"], fwd["units"], fwd["zs"], fwd["folds"])


def rpn_backward(canvas, wc, wn, bn, fwd, dy):
    """-> ({key: gradient} for the 57 tensors of PARAM_KEYS, dcanvas), float64, from a forward's tensors and dy [nb,320,H,W]."""
    y, taps, units, zs, folds, stats = (fwd[k] for k in ("y", "taps", "units", "zs", "folds", "stats"))
    grads = {}

    def put(key, dw, dscale, dshift):
        p = bn_prefix(key)
        grads[key] = dw
        grads[p + ".weight"], grads[p + ".bias"] = affine_grad(dscale, dshift, *stats[p][:2])

    def args(key):
        p = bn_prefix(key)
        return (*folds[p], *stats[p][:2])

    dxn = []
    for b in range(3):
        sl = slice(N.COFF[b], N.COFF[b] + N.CUP[b])
        sc, _, m, v = args(NECK_KEYS[b])
        dw, dx, ds, dh = branch_backward(taps[b], wn[b], sc, m, v, y[:, sl], np.asarray(dy)[:, sl])
        put(NECK_KEYS[b], dw, ds, dh)
        dxn.append(dx)
    g = None
    for b, mods in reversed(RPN_TABLE):
        keys = CONV_KEYS[W0[b]:W0[b] + 1 + sum(mods)]
        g = dxn[b] if g is None else dxn[b] + g
        i = sum(mods)
        for n in reversed(mods):
            i -= n
            skip = g
            for j in ((i + 1, i) if n == 2 else (i,)):
                k = keys[1 + j]
                dw, g, ds, dh = unit_backward(units[b][j], wc[W0[b] + 1 + j], *args(k), g, dskip=skip if j == i else None)
                put(k, dw, ds, dh)
        dw, g, ds, dh = down_backward(canvas if b == 0 else taps[b - 1], wc[W0[b]], zs[b], *args(keys[0]), g)
        put(keys[0], dw, ds, dh)
    return grads, g
