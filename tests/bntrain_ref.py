"""CPU restatement (numpy, float64) of fine-tuning the BatchNorm RPN with frozen statistics: every BatchNorm2d(eps 1e-3) in eval mode
is the per-channel affine norm(v) = scale v + shift, scale = gamma / sqrt(running_var + 1e-3), shift = beta - running_mean scale.  The
three backward primitives (csrc/block_train.hip, down_train.hip, neck_train.hip: pp_*_backward_affine) and the whole chain, wired by
the table of rpntrain_ref.  Pinned to the reference's own autograd by tests/golden/bntrain_small.npz (tests/test_bntrain_cpu.py); the
GPU tests use it where no golden can be stored.

The a-priori bounds (`*_bounds`) are for a float32 implementation working from the same float32 inputs, U = 2^-24, first order, inflated
by 1 %.  The affine norm makes them short: fma(v, scale, shift) is rounded once and keeps the sign of the exact value, so the ReLU mask
of a float32 evaluation IS the float64 mask (no near-ties), and a = max(fma, 0) is off by U |a| at most."""
import numpy as np

import blocktrain_ref as B
import downtrain_ref as D
import necktrain_ref as N
from rpntrain_ref import CONV_KEYS, NECK_KEYS, RPN_TABLE, W0

EPS = 1e-3
U32 = 2.0 ** -24
U64 = 2.0 ** -53


def bn_prefix(conv_key):
    """The BatchNorm2d layer of a convolution or upsampler: behind a strided convolution or an upsampler, in front of a unit's."""
    stem, idx, _ = conv_key.rsplit(".", 2)
    return stem + "." + {"0": "1", "2": "0", "5": "3"}[idx]


# the nineteen BatchNorm2d layers in state_dict order, and the reference's named_parameters() order of the 57 RPN tensors
LAYER_KEYS = tuple(k for b in range(3) for k in CONV_KEYS[W0[b]:W0[b] + 1 + sum(RPN_TABLE[b][1])] + (NECK_KEYS[b],))
BN_PREFIXES = tuple(bn_prefix(k) for k in LAYER_KEYS)
PARAM_KEYS = tuple(n for k in LAYER_KEYS for n in
                   ((k, bn_prefix(k) + ".weight", bn_prefix(k) + ".bias") if k.rsplit(".", 2)[1] == "0" else
                    (bn_prefix(k) + ".weight", bn_prefix(k) + ".bias", k)))


def fold(gamma, beta, rm, rv):
    """-> scale, shift in float64."""
    gamma, beta, rm, rv = (np.asarray(t, np.float64) for t in (gamma, beta, rm, rv))
    s = gamma / np.sqrt(rv + EPS)
    return s, beta - rm * s


def fold32(gamma, beta, rm, rv):
    """The fold as the library rounds it: the float64 expression, each value rounded once to float32."""
    s = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(rv, np.float64) + EPS)
    return s.astype(np.float32), (np.asarray(beta, np.float64) - np.asarray(rm, np.float64) * s).astype(np.float32)


def affine_grad(dscale, dshift, rm, rv):
    """The sums of a primitive -> dgamma, dbeta."""
    r = 1.0 / np.sqrt(np.asarray(rv, np.float64) + EPS)
    return r * (np.asarray(dscale, np.float64) - np.asarray(rm, np.float64) * dshift), np.asarray(dshift, np.float64)


def ch(v):
    return np.asarray(v, np.float64)[None, :, None, None]


def aff(v, scale, shift):
    return np.asarray(v, np.float64) * ch(scale) + ch(shift)


def sums(g, v):
    return (g * v).sum((0, 2, 3)), g.sum((0, 2, 3))


# ------------------------------------------------------------------ unit: affine -> ReLU -> Conv3x3
def unit_forward(u, w, scale, shift):
    return B.conv3(np.maximum(aff(u, scale, shift), 0.0), np.asarray(w, np.float64))


def unit_backward(u, w, scale, shift, dz, dskip=None):
    """-> dw, du, dscale = sum g u, dshift = sum g (float64)."""
    u64, w64, dz64 = (np.asarray(t, np.float64) for t in (u, w, dz))
    a = np.maximum(aff(u64, scale, shift), 0.0)
    g = B.conv3_dgrad(dz64, w64) * (a > 0)
    du = ch(scale) * g
    if dskip is not None:
        du = du + np.asarray(dskip, np.float64)
    return (B.conv3_wgrad(dz64, a), du) + sums(g, u64)


def unit_bounds(u, w, scale, shift, dz, dskip=None):
    """-> (dw, du, dscale, dshift), (bw, bu, bs, bh).  dw sums K_w = nb h w products dz a32, |a32 - a| <= U |a|; da sums K_x = 9 C
    products of exact inputs, eda := K_x U sum |w dz| + U |da|; du = fl(scale g) (+ dskip, one more rounding); the two sums are float64
    sums of float32 g (and the exact float64 product g u): they inherit eda and add n 2^-53 sum |terms|."""
    u64, w64, dz64 = (np.asarray(t, np.float64) for t in (u, w, dz))
    nb, C, h, wd = u64.shape
    dw, du, ds, dh = unit_backward(u, w, scale, shift, dz, dskip)
    a = np.maximum(aff(u64, scale, shift), 0.0)
    mask = a > 0
    bw = (nb * h * wd + 1) * U32 * B.conv3_wgrad(np.abs(dz64), a) + U32 * np.abs(dw) + 1e-45
    da = B.conv3_dgrad(dz64, w64)
    eg = (9 * C * U32 * B.conv3_dgrad(np.abs(dz64), np.abs(w64)) + U32 * np.abs(da)) * mask
    g = da * mask
    asc = np.abs(ch(scale))
    bu = asc * eg + U32 * asc * np.abs(g) + (U32 * np.abs(du) if dskip is not None else 0.0) + 1e-45
    n = nb * h * wd
    bs = (eg * np.abs(u64)).sum((0, 2, 3)) + n * U64 * (np.abs(g * u64)).sum((0, 2, 3)) + 1e-300
    bh = eg.sum((0, 2, 3)) + n * U64 * np.abs(g).sum((0, 2, 3)) + 1e-300
    return (dw, du, ds, dh), tuple(1.01 * b for b in (bw, bu, bs, bh))


# ------------------------------------------------------------------ stage: Conv3x3 stride 2 -> affine -> ReLU
def down_forward(x, w, scale, shift, return_z=False):
    z = D.conv_s2(np.asarray(x, np.float64), np.asarray(w, np.float64))
    h = np.maximum(aff(z, scale, shift), 0.0)
    return (h, z) if return_z else h


def down_backward(x, w, z, scale, shift, dy):
    """-> dw, dx, dscale = sum g z, dshift = sum g (float64); z is the conv output the forward stored."""
    x64, w64, z64 = (np.asarray(t, np.float64) for t in (x, w, z))
    g = np.asarray(dy, np.float64) * (aff(z64, scale, shift) > 0)
    dz = ch(scale) * g
    return (D.conv_s2_wgrad(dz, x64), D.conv_s2_dgrad(dz, w64, *x64.shape[-2:])) + sums(g, z64)


def down_bounds(x, w, z, scale, shift, dy):
    """g = dy [mask] is exact, dz32 = fl(scale g) is off by U |dz|; dw sums K_w = nb ho wo products, dx at most K_x = 4 Cout; the two
    sums are float64 sums of exact products: n 2^-53 sum |terms|."""
    x64, w64, z64 = (np.asarray(t, np.float64) for t in (x, w, z))
    nb, cout, ho, wo = z64.shape
    hin, win = x64.shape[-2:]
    dw, dx, ds, dh = down_backward(x, w, z, scale, shift, dy)
    g = np.asarray(dy, np.float64) * (aff(z64, scale, shift) > 0)
    adz = np.abs(ch(scale) * g)
    bw = (nb * ho * wo + 1) * U32 * D.conv_s2_wgrad(adz, np.abs(x64)) + U32 * np.abs(dw) + 1e-45
    bx = (4 * cout + 1) * U32 * D.conv_s2_dgrad(adz, np.abs(w64), hin, win) + U32 * np.abs(dx) + 1e-45
    n = nb * ho * wo
    bs = n * U64 * np.abs(g * z64).sum((0, 2, 3)) + 1e-300
    bh = n * U64 * np.abs(g).sum((0, 2, 3)) + 1e-300
    return (dw, dx, ds, dh), tuple(1.01 * b for b in (bw, bx, bs, bh))


# ------------------------------------------------------------------ branch: ConvTranspose(k = s) -> affine -> ReLU
def branch_forward(x, w, scale, shift):
    return np.maximum(aff(N.conv_t(x, w), scale, shift), 0.0)


def branch_backward(x, w, scale, y, dy, bounds=False):
    """y / dy: the branch's channel slice of rpn_out and of its gradient; the mask is the GIVEN y -> dw, dx, dscale = sum g Z,
    dshift = sum g (float64).  bounds=True: and their a-priori bounds.  Z32 is a float32 sum of Cin products, |Z32 - Z| <= (Cin + 1) U
    sum |w x|; g is exact, dZ32 = fl(scale g); dw sums K_w = nb h w products, dx K_x = Cup s s."""
    x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    nb, cin, h, wd = x64.shape
    s = w64.shape[2]
    Z = N.conv_t(x64, w64)
    g = np.asarray(dy, np.float64) * (np.asarray(y) > 0)
    dZr = N.to_rows(ch(scale) * g, s)
    X, Wr = x64.reshape(nb, cin, -1), w64.reshape(cin, -1)
    dw = np.matmul(X, dZr.transpose(0, 2, 1)).sum(0).reshape(w64.shape)
    dx = np.matmul(Wr[None], dZr).reshape(x64.shape)
    out = (dw, dx) + sums(g, Z)
    if not bounds:
        return out
    aw = np.matmul(np.abs(X), np.abs(dZr).transpose(0, 2, 1)).sum(0).reshape(w64.shape)
    ax = np.matmul(np.abs(Wr)[None], np.abs(dZr)).reshape(x64.shape)
    eZ = (cin + 1) * U32 * N.conv_t(np.abs(x64), np.abs(w64))
    n = nb * Z.shape[2] * Z.shape[3]
    bw = (nb * h * wd + 1) * U32 * aw + U32 * np.abs(dw) + 1e-45
    bx = (w64.shape[1] * s * s + 1) * U32 * ax + U32 * np.abs(dx) + 1e-45
    bs = (np.abs(g) * eZ).sum((0, 2, 3)) + n * U64 * np.abs(g * Z).sum((0, 2, 3)) + 1e-300
    bh = n * U64 * np.abs(g).sum((0, 2, 3)) + 1e-300
    return out, tuple(1.01 * b for b in (bw, bx, bs, bh))


# ------------------------------------------------------------------ the whole RPN
def rpn_forward(canvas, wc, wn, bn):
    """canvas [nb,64,gx,gy], wc the sixteen convolutions in CONV_KEYS order, wn the three upsamplers, bn {BatchNorm prefix: (gamma,
    beta, running_mean, running_var)} -> dict: y, taps, units, zs as rpntrain_ref.rpn_forward, and folds {prefix: (scale, shift)}."""
    folds = {p: fold(*bn[p]) for p in BN_PREFIXES}
    x = np.asarray(canvas, np.float64)
    taps, units, zs, ys = [], [], [], []
    for b, mods in RPN_TABLE:
        keys = CONV_KEYS[W0[b]:W0[b] + 1 + sum(mods)]
        w = [np.asarray(t, np.float64) for t in wc[W0[b]:W0[b] + 1 + sum(mods)]]
        U = lambda r, i: unit_forward(r, w[i], *folds[bn_prefix(keys[i])])  # noqa: E731
        r, z = down_forward(x, w[0], *folds[bn_prefix(keys[0])], return_z=True)
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
        ys.append(branch_forward(x, wn[b], *folds[bn_prefix(NECK_KEYS[b])]))
    return dict(y=np.concatenate(ys, 1), taps=taps, units=units, zs=zs, folds=folds)


def relu_masks(y, units, zs, folds):
    """The branch every ReLU takes, from the tensors a forward hands out -> {site name: bool array}."""
    out = {}
    for b, mods in RPN_TABLE:
        keys = CONV_KEYS[W0[b]:W0[b] + 1 + sum(mods)]
        out[f"stage{b}"] = aff(zs[b], *folds[bn_prefix(keys[0])]) > 0
        for k, u in enumerate(units[b]):
            out[f"unit{b}.{k}"] = aff(u, *folds[bn_prefix(keys[1 + k])]) > 0
        out[f"up{b}"] = np.asarray(y)[:, N.COFF[b]:N.COFF[b] + N.CUP[b]] > 0
    return out


def rpn_backward(canvas, wc, wn, bn, fwd, dy):
    """-> ({key: gradient} for the 57 tensors of PARAM_KEYS, dcanvas), float64, from a forward's tensors and dy [nb,320,H,W]."""
    y, taps, units, zs, folds = fwd["y"], fwd["taps"], fwd["units"], fwd["zs"], fwd["folds"]
    grads = {}

    def put(key, dw, dscale, dshift):
        p = bn_prefix(key)
        grads[key] = dw
        grads[p + ".weight"], grads[p + ".bias"] = affine_grad(dscale, dshift, bn[p][2], bn[p][3])

    dxn = []
    for b in range(3):
        sl = slice(N.COFF[b], N.COFF[b] + N.CUP[b])
        dw, dx, ds, dh = branch_backward(taps[b], wn[b], folds[bn_prefix(NECK_KEYS[b])][0], y[:, sl], np.asarray(dy)[:, sl])
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
                dw, g, ds, dh = unit_backward(units[b][j], wc[W0[b] + 1 + j], *folds[bn_prefix(k)], g, dskip=skip if j == i else None)
                put(k, dw, ds, dh)
        dw, g, ds, dh = down_backward(canvas if b == 0 else taps[b - 1], wc[W0[b]], zs[b], *folds[bn_prefix(keys[0])], g)
        put(keys[0], dw, ds, dh)
    return grads, g
