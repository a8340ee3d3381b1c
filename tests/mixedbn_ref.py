"""CPU side of the mixed-precision BatchNorm backwards (pp_{unit,down,neck}_backward_affine_mp / _bn_mp, csrc/block_train16.hip,
down_train16.hip, neck_train16.hip): an emulation of the modes' arithmetic, the element-wise a-priori bounds that the fp32 bounds of
bntrain_ref (form "affine": frozen statistics) and bnbatch_ref (form "batch": batch statistics) become when the operands of the two
gradient products are 16-bit, and the exact-arithmetic inputs of the indexing test.  bntrain_ref, bnbatch_ref, mixedtrain_ref and
mixedstage_ref are imported and left as they are.

Modes (mixedtrain_ref.MODES: eps the relative error of a product of two 16-bit operands, m the MFMAs per product), U = 2^-24.

Unit, both forms.  a = max(fma(u, scale, shift), 0) is evaluated in fp32 and rounded or split, dz and w likewise; the mask is fp32's
(fma rounds once and keeps the sign), so there are no near-ties.  With bw and eg the terms of bntrain_ref.unit_bounds:
  bw_mixed = bw + 1.01 (eps + (m - 1) nb N U) conv3_wgrad(|dz|, a)
  eg_mixed = eg + (eps + (m - 1) 9 C U) conv3_dgrad(|dz|, |w|) [mask]
and bu, bs, bh are the form's own expressions with eg_mixed in place of eg: bntrain_ref.unit_bounds' lines (affine),
bnbatch_ref.norm_backward_bound (batch).  bf16x3 adds 2^-126 sum |other operand| for lo parts the MFMA may flush, as mixedtrain_ref.

Stage and branch.  dz / dZ is the fp32 path's, so the form's fp32 bound carries the product terms of mixedstage_ref._mixed: K = nb x
positions for dw, 4 Cout (stage) or Cup s s (branch) for dx, over sum |dz| |x| and sum |w| |dz| of the exact dz.  The operand error is
relative to the fp32 dz, which lies within e_dz of the exact one; eps e_dz sum |.| is below the 1 % by which both reference modules
inflate their own e_dz term (eps < 2^-7 < 0.01).  dscale / dshift are the fp32 path's bits: their bounds are the fp32 ones."""
import numpy as np

import blocktrain_ref as B
import bnbatch_ref as RB
import bntrain_ref as RA
import mixedstage_ref as S
import mixedtrain_ref as M
from mixedtrain_ref import MODES, TINY, bf16_round, bf16_split  # noqa: F401

U32, U64 = RA.U32, RA.U64
FORMS = ("affine", "batch")
_f64 = lambda t: np.asarray(t, np.float64)  # noqa: E731

# the cases of tests/test_mixedbn_gpu.py, cleared by tests/test_mixedbn_cpu.py
UNIT_SHAPES = [(64, 33, 17, 1), (128, 20, 18, 2), (256, 25, 9, 3), (256, 1, 7, 2), (256, 3, 2, 2)]  # test_mixedtrain_gpu.SHAPES' (C, h, w, nb)
UNIT_LARGE = (64, 130, 127, 1)  # the 16 510-position plane, once per form
UNIT_APART = (64, 33, 17, 1)    # "the modes are told apart"
EXACT_UNITS = [(64, 13, 11, 2), (128, 13, 11, 2), (256, 13, 11, 2)]                 # row pitch 13: no multiple of 8
EXACT_DOWNS = [(64, 64, 13, 11, 2), (64, 128, 13, 11, 2), (128, 256, 13, 11, 2)]  # (cin, cout, hin, win, nb)
EXACT_NECK = (12, 20, 2)  # (H, W, nb) of the level-0 map


def norm_params(rng, C):
    """gamma, beta, running_mean, running_var: test_bntrain_gpu.norm_params."""
    return (rng.uniform(0.5, 1.5, C).astype(np.float32), (rng.standard_normal(C) * 0.1).astype(np.float32),
            (rng.standard_normal(C) * 0.1).astype(np.float32), rng.uniform(0.5, 1.5, C).astype(np.float32))


def norm_of(v, rng, C, form):
    """The norm's tensors as the library holds them (float32): (scale, shift) of drawn running statistics for the affine form, (scale,
    shift, mean, var) of v's batch statistics for the batch form."""
    if form == "affine":
        return RA.fold32(*norm_params(rng, C))
    mean, var = RB.stats32(v)
    return (*RB.fold32(*norm_params(rng, C)[:2], mean, var), mean, var)


def unit_case(C, h, w, nb, form, seed=None):
    """u, w, norm, dz, dskip."""
    rng = np.random.default_rng(900 + C + h if seed is None else seed)
    u = rng.standard_normal((nb, C, h, w)).astype(np.float32)
    wt = (rng.standard_normal((C, C, 3, 3)) * 0.05).astype(np.float32)
    dz, dskip = rng.standard_normal((nb, C, h, w)).astype(np.float32), rng.standard_normal((nb, C, h, w)).astype(np.float32)
    return u, wt, norm_of(u, rng, C, form), dz, dskip


def down_case(cin, cout, hin, win, nb, form):
    x, w, z, dy = S.down_case(cin, cout, hin, win, nb)
    return x, w, z, norm_of(z, np.random.default_rng(910 + cout + hin), cout, form), dy


def neck_case(H, W, nb, form):
    """xs, ws, norms (per branch), y [nb,320,H,W] (the float32 cast of the float64 forward through each branch's norm), dy."""
    import necktrain_ref as N
    xs, ws, _, dy = S.neck_case(H, W, nb)
    rng = np.random.default_rng(920 + H)
    norms = [norm_of(N.conv_t(_f64(xs[b]), _f64(ws[b])), rng, N.CUP[b], form) for b in range(3)]
    y = np.concatenate([RA.branch_forward(xs[b], ws[b], norms[b][0], norms[b][1]) for b in range(3)], 1).astype(np.float32)
    return xs, ws, norms, y, dy


# ------------------------------------------------------------------ emulation: operands as the kernels take them, float64 products
def a_fp32(u, scale, shift):
    """a = max(fma(u, scale, shift), 0) in float32: the float64 product of two float32 values is exact, the sum is rounded to float64
    and then to float32 (a double rounding that differs from the fma's single one by at most 2^-29 relative)."""
    v = (np.asarray(u, np.float32).astype(np.float64) * RA.ch(np.asarray(scale, np.float32)) + RA.ch(np.asarray(shift, np.float32))).astype(np.float32)
    return np.maximum(v, np.float32(0))


def unit_emulate(u, w, norm, dz, mode, dskip=None):
    """-> dw, du, dscale, dshift: a in float32, operands rounded (bf16) or split (bf16x3), products and sums in float64, the form's norm
    backward in float64."""
    a = a_fp32(u, norm[0], norm[1])
    dw = S._product(M.wgrad, dz, a, mode)
    da = S._product(B.conv3_dgrad, dz, w, mode)
    g, u64 = da * (a > 0), _f64(u)
    if len(norm) == 2:
        du, (ds, dh) = RA.ch(norm[0]) * g, RA.sums(g, u64)
    else:
        du, ds, dh, _ = RB.norm_backward(g, u64, norm[0], norm[2], norm[3])
    return dw, (du if dskip is None else du + _f64(dskip)), ds, dh


def _dz32(v, norm, dy, mask):
    """The fp32 dz every mode reads: the form's float64 expression rounded once to float32."""
    g = _f64(dy) * mask
    if len(norm) == 2:
        return (RA.ch(norm[0]) * g).astype(np.float32)
    return RB.norm_backward(g, _f64(v), norm[0], norm[2], norm[3])[0].astype(np.float32)


def down_emulate(x, w, z, norm, dy, mode):
    hin, win = np.shape(x)[-2:]
    dz = _dz32(z, norm, dy, RA.aff(z, norm[0], norm[1]) > 0)
    return S._product(S.wgrad_s2, dz, x, mode), S._product(lambda a, b: S.D.conv_s2_dgrad(a, b, hin, win), dz, w, mode)


def neck_emulate(x, w, norm, y, dy, mode):
    """y, dy: the branch's channel slices."""
    nb, cin = np.shape(x)[:2]
    s = np.shape(w)[2]
    dz = S.N.to_rows(_dz32(S.N.conv_t(_f64(x), _f64(w)), norm, dy, np.asarray(y) > 0), s)
    X, Wr = np.asarray(x, np.float32).reshape(nb, cin, -1), np.asarray(w, np.float32).reshape(cin, -1)
    dw = S._product(lambda a, b: np.matmul(b, a.transpose(0, 2, 1)).sum(0), dz, X, mode).reshape(np.shape(w))
    return dw, S._product(lambda a, b: np.matmul(b[None], a), dz, Wr, mode).reshape(np.shape(x))


# ------------------------------------------------------------------ bounds
def unit_terms(u, w, norm, dz):
    """What the unit bounds are made of and neither the mode nor dskip touches."""
    u64, w64, dz64 = _f64(u), _f64(w), _f64(dz)
    a = np.maximum(RA.aff(u64, norm[0], norm[1]), 0.0)
    adz = np.abs(dz64)
    da = B.conv3_dgrad(dz64, w64)
    return dict(u=u64, a=a, mask=a > 0, dw=M.wgrad(dz64, a), aw=M.wgrad(adz, a), da=da, awz=B.conv3_dgrad(adz, np.abs(w64)),
                zmax=float(adz.max()), amax=float(a.max()), wmax=float(np.abs(w64).max()))


def unit_bounds_mixed(u, w, norm, dz, mode, dskip=None, terms=None):
    """-> (dw, du, dscale, dshift) in float64 from the exact inputs and (bw, bu, bs, bh), the element-wise bounds of a mode's deviation
    from them; mode "fp32" gives bntrain_ref.unit_bounds / bnbatch_ref.unit_bounds themselves (tests/test_mixedbn_cpu.py holds them
    together)."""
    t = unit_terms(u, w, norm, dz) if terms is None else terms
    eps, m = (0.0, 1) if mode == "fp32" else MODES[mode]
    nb, C, h, wd = np.shape(u)
    n = nb * h * wd
    u64, mask, da = t["u"], t["mask"], t["da"]
    bw = 1.01 * ((n + 1) * U32 * t["aw"] + U32 * np.abs(t["dw"]) + 1e-45) + 1.01 * (eps + (m - 1) * n * U32) * t["aw"]
    eg = (9 * C * U32 * t["awz"] + U32 * np.abs(da)) * mask + (eps + (m - 1) * 9 * C * U32) * t["awz"] * mask
    if m == 3:
        bw = bw + 1.01 * TINY * n * (t["zmax"] + t["amax"])
        eg = eg + TINY * 9 * C * (t["zmax"] + t["wmax"]) * mask
    g = da * mask
    bs = (eg * np.abs(u64)).sum((0, 2, 3)) + n * U64 * np.abs(g * u64).sum((0, 2, 3)) + 1e-300
    bh = eg.sum((0, 2, 3)) + n * U64 * np.abs(g).sum((0, 2, 3)) + 1e-300
    if len(norm) == 2:
        asc = np.abs(RA.ch(norm[0]))
        du = RA.ch(norm[0]) * g
        ds, dh = RA.sums(g, u64)
        bu = asc * eg + U32 * asc * np.abs(g)
    else:
        du, ds, dh, _ = RB.norm_backward(g, u64, norm[0], norm[2], norm[3])
        bu = RB.norm_backward_bound(g, eg, u64, 0.0, norm[0], norm[2], norm[3], bs, bh)
    if dskip is not None:
        du = du + _f64(dskip)
        bu = bu + U32 * np.abs(du)
    return (t["dw"], du, ds, dh), (bw, 1.01 * (bu + 1e-45), 1.01 * bs, 1.01 * bh)


def down_terms(x, w, z, norm, dy):
    """The form's fp32 bounds and the two sums of absolute products that mixedstage_ref._mixed adds to them (mode-independent)."""
    fp32 = RA.down_bounds(x, w, z, *norm, dy) if len(norm) == 2 else RB.down_bounds(x, w, z, *norm, dy)
    (dw, dx, ds, dh), (bw, bx, bs, bh) = fp32
    hin, win = np.shape(x)[-2:]
    g = _f64(dy) * (RA.aff(z, norm[0], norm[1]) > 0)
    adz = np.abs(RA.ch(norm[0]) * g if len(norm) == 2 else RB.norm_backward(g, _f64(z), norm[0], norm[2], norm[3])[0])
    nb, cout, ho, wo = adz.shape
    ax_, aw_ = np.abs(_f64(x)), np.abs(_f64(w))
    return dict(out=(dw, dx, ds, dh), bw=bw, bx=bx, bs=bs, bh=bh, aw=S.wgrad_s2(adz, ax_), ax=S.D.conv_s2_dgrad(adz, aw_, hin, win),
                Kw=nb * ho * wo, Kx=4 * cout, zmax=float(adz.max()), xmax=float(ax_.max()), wmax=float(aw_.max()))


def neck_terms(x, w, norm, y, dy):
    """As down_terms for one branch; y, dy are its channel slices."""
    if len(norm) == 2:
        out, (bw, bx, bs, bh) = RA.branch_backward(x, w, norm[0], y, dy, bounds=True)
    else:
        out, (bw, bx, bs, bh) = RB.branch_backward(x, w, norm[0], norm[2], norm[3], y, dy, bounds=True)
    x64, w64 = _f64(x), _f64(w)
    nb, cin, h, wd = x64.shape
    s = w64.shape[2]
    g = _f64(dy) * (np.asarray(y) > 0)
    dZ = RA.ch(norm[0]) * g if len(norm) == 2 else RB.norm_backward(g, S.N.conv_t(x64, w64), norm[0], norm[2], norm[3])[0]
    adz = np.abs(S.N.to_rows(dZ, s))
    aw = np.matmul(np.abs(x64.reshape(nb, cin, -1)), adz.transpose(0, 2, 1)).sum(0).reshape(w64.shape)
    ax = np.matmul(np.abs(w64.reshape(cin, -1))[None], adz).reshape(x64.shape)
    return dict(out=out, bw=bw, bx=bx, bs=bs, bh=bh, aw=aw, ax=ax, Kw=nb * h * wd, Kx=int(np.prod(w64.shape[1:])),
                zmax=float(adz.max()), xmax=float(np.abs(x64).max()), wmax=float(np.abs(w64).max()))


def stage_bounds_mixed(t, mode):
    """down_terms / neck_terms -> (dw, dx, dscale, dshift), (bw, bx, bs, bh) of a mode ("fp32": the form's own bounds)."""
    bw, bx = S._mixed(t, mode)
    return t["out"], (bw, bx, t["bs"], t["bh"])


def worst(got, want, bound):
    return S.worst(got, want, bound)


# ------------------------------------------------------------------ exact data: every operand survives bf16, every sum is exact in fp32
def _ints(rng, shape, lo, hi, scale):
    return (rng.integers(lo, hi + 1, shape) * scale).astype(np.float32)


def exact_norm(rng, C, v, form):
    """scale in {+-1/2, +-1, +-2}, shift integers in [-4, 4] x 2^-2; the batch form adds the batch statistics of v as given values."""
    scale = (rng.choice([0.5, 1.0, 2.0], C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    shift = _ints(rng, C, -4, 4, 0.25)
    return (scale, shift) if form == "affine" else (scale, shift, *RB.stats32(v))


def exact_unit(C, h, w, nb, form):
    """u integers in [-8, 8] x 2^-2, dz integers in [-4, 4] x 2^-2, weights integers in [-3, 3] x 2^-4 -> u, w, norm, dz."""
    rng = np.random.default_rng(1000 + C)
    u, dz = _ints(rng, (nb, C, h, w), -8, 8, 0.25), _ints(rng, (nb, C, h, w), -4, 4, 0.25)
    return u, _ints(rng, (C, C, 3, 3), -3, 3, 0.0625), exact_norm(rng, C, u, form), dz


def exact_down(cin, cout, hin, win, nb, form="affine"):
    """x, z as u above (z is a given tensor: the mask is fma(z, scale, shift) > 0 whatever the convolution would give) -> x, w, z, norm, dy."""
    rng = np.random.default_rng(1100 + cout)
    ho, wo = (hin + 1) // 2, (win + 1) // 2
    x, z = _ints(rng, (nb, cin, hin, win), -8, 8, 0.25), _ints(rng, (nb, cout, ho, wo), -8, 8, 0.25)
    return x, _ints(rng, (cout, cin, 3, 3), -3, 3, 0.0625), z, exact_norm(rng, cout, z, form), _ints(rng, z.shape, -4, 4, 0.25)


def exact_neck(H, W, nb, form="affine"):
    """-> xs, ws, norms, y (the mask: y > 0 on about half the elements), dy."""
    import necktrain_ref as N
    rng = np.random.default_rng(1200 + H)
    xs = [_ints(rng, (nb, N.CIN[b], H >> b, W >> b), -8, 8, 0.25) for b in range(3)]
    ws = [_ints(rng, (N.CIN[b], N.CUP[b], 1 << b, 1 << b), -3, 3, 0.0625) for b in range(3)]
    norms = [exact_norm(rng, N.CUP[b], N.conv_t(_f64(xs[b]), _f64(ws[b])), form) for b in range(3)]
    return xs, ws, norms, _ints(rng, (nb, 320, H, W), -1, 1, 1.0), _ints(rng, (nb, 320, H, W), -4, 4, 0.25)


def exact_margin(a, b, terms):
    """A product of operands a, b summed over `terms` terms in any order stays exact in float32 when every partial sum is an integer
    multiple of the product of the operands' grains and below 2^24 of them -> terms x max |a| max |b| / (grain a x grain b) / 2^24,
    which must be below 1."""
    return terms * float(np.abs(_f64(a)).max()) * float(np.abs(_f64(b)).max()) / (_lsb(a) * _lsb(b)) / 2.0 ** 24


def _lsb(t):
    """The largest power of two that divides every element of t."""
    v = np.abs(_f64(t).reshape(-1))
    v = v[v > 0]
    g = 2.0 ** 60
    while np.any((v / g) % 1.0 != 0):
        g /= 2.0
    return g
