"""CPU restatement (numpy, float64) of the backbone's pre-activation Resnet unit, InstanceNorm2d(eps 1e-3, no affine) -> ReLU ->
Conv2d(C -> C, 3 x 3, pad 1, no bias), forward and backward (csrc/block_train.hip).  Pinned to the reference's own autograd by
tests/golden/blocktrain_small.npz (tests/test_blocktrain_cpu.py); the GPU tests use it where no golden can be stored.

For a frame and input channel, N = h w: mean = sum u / N, rstd = 1 / sqrt(sum u^2 / N - mean^2 + 1e-3), xhat = (u - mean) rstd,
a = max(xhat, 0), z[co, p] = sum_{ci, ky, kx} w[co][ci][ky][kx] a[ci, py + ky - 1, px + kx - 1] with zero padding."""
import numpy as np

EPS = 1e-3
U32 = 2.0 ** -24


def norm(u):
    """-> xhat, mean, rstd in float64."""
    u = np.asarray(u, np.float64)
    mean = u.mean((2, 3), keepdims=True)
    rstd = 1.0 / np.sqrt(u.var((2, 3), keepdims=True) + EPS)
    return (u - mean) * rstd, mean, rstd


def shifted(t, dy, dx):
    """s[..., y, x] = t[..., y + dy, x + dx], zero outside."""
    h, w = t.shape[-2:]
    p = np.pad(t, [(0, 0)] * (t.ndim - 2) + [(1, 1), (1, 1)])
    return p[..., 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]


def conv3(a, w):
    """a [nb, C, h, w], w [Co, C, 3, 3] -> [nb, Co, h, w], float64."""
    out = 0.0
    for ky in range(3):
        for kx in range(3):
            out = out + np.einsum("oc,nchw->nohw", w[:, :, ky, kx], shifted(a, ky - 1, kx - 1), optimize=True)
    return out


def conv3_dgrad(dz, w):
    """da[ci, q] = sum_{co, ky, kx} w[co][ci][ky][kx] dz[co, qy - ky + 1, qx - kx + 1]."""
    out = 0.0
    for ky in range(3):
        for kx in range(3):
            out = out + np.einsum("oc,nohw->nchw", w[:, :, ky, kx], shifted(dz, 1 - ky, 1 - kx), optimize=True)
    return out


def conv3_wgrad(dz, a):
    """dw[co][ci][ky][kx] = sum_{f, p} dz[f, co, p] a[f, ci, py + ky - 1, px + kx - 1]."""
    dw = np.empty((dz.shape[1], a.shape[1], 3, 3))
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = np.einsum("nohw,nchw->oc", dz, shifted(a, ky - 1, kx - 1), optimize=True)
    return dw


def unit_forward(u, w, return_xhat=False):
    """z = conv3(relu(instance_norm(u)), w) in float64 (and xhat)."""
    xhat, _, _ = norm(u)
    z = conv3(np.maximum(xhat, 0.0), np.asarray(w, np.float64))
    return (z, xhat) if return_xhat else z


def unit_backward(u, w, dz, dskip=None):
    """u, dz, dskip [nb, C, h, w], w [C, C, 3, 3] -> dw [C, C, 3, 3] summed over the frames, du [nb, C, h, w], float64."""
    w64, dz64 = np.asarray(w, np.float64), np.asarray(dz, np.float64)
    xhat, _, rstd = norm(u)
    a = np.maximum(xhat, 0.0)
    dw = conv3_wgrad(dz64, a)
    Gr = conv3_dgrad(dz64, w64) * (a > 0)
    du = rstd * (Gr - Gr.mean((2, 3), keepdims=True) - xhat * (Gr * xhat).mean((2, 3), keepdims=True))
    if dskip is not None:
        du = du + np.asarray(dskip, np.float64)
    return dw, du


def near_ties(u, width):
    """Elements whose float64 |xhat| < width: there the ReLU mask of a float32 evaluation may differ."""
    return np.abs(norm(u)[0]) < width


def tie_free(u, width=1e-4):
    """A float32 copy of u in which no element has |xhat| < width: near-ties are pushed 1e-2 standard deviations away from their
    plane's mean (which moves the plane's statistics by ~1e-2 / N of that, so a second round is rarely needed).  Deterministic.
    Choosing a seed instead works for the fixture's few thousand elements only: a standard normal element is a near-tie with
    probability 8e-5, so the 172800 elements of the 256 x 25 x 9 x 3 case hold 14 of them on average and one seed in a million none."""
    u = np.array(u, np.float32)
    for _ in range(8):
        xhat, _, rstd = norm(u)
        t = np.abs(xhat) < width
        if not t.any():
            return u
        u = np.where(t, u + np.where(xhat >= 0, 1e-2, -1e-2) / rstd, u).astype(np.float32)
    raise AssertionError("tie_free: near-ties left")


def grad_bounds(u, w, dz, dskip=None, tie=1e-5):
    """-> dw, du (float64), element-wise a-priori bounds bw, bu of |dw32 - dw| and |du32 - du| for a float32 implementation working
    from the same float32 inputs, and the near-tie set t = [|xhat64| < tie].  First-order bounds, inflated by 1 % for the second-order
    terms; U = 2^-24.

    xhat32 = fl(fl(u - fl(mean)) fl(rstd)) with mean and rstd from float64 sums:  |xhat32 - xhat| <= ex := U (rstd |mean| +
    4 max(1, max |xhat|)) per plane (the rounded mean moved by rstd, three roundings of a quantity of size |xhat|, one spare for the
    float64 statistics).  ReLU is 1-Lipschitz, so |a32 - a| <= ex too.
    dw sums K_w = nb h w products dz a32 in float32 in any order:  |dw err| <= K_w U sum |dz a| + ex sum |dz| + U |dw|.
    da sums K_x = 9 C products of exact inputs:                    eda := K_x U sum |w dz| + U |da|.
    Gr = da [a > 0]; c1 = mean(Gr), c2 = mean(Gr xhat) in float64 from float32 values, rounded once:
        ec1 := mean(eGr) + U |c1|,    ec2 := mean(eGr |xhat| + |Gr| ex) + U |c2|.
    du = fl(rstd fl(fl(Gr - c1) - fl(xhat c2))) (+ dskip, one more rounding):
        |du err| <= rstd (eGr + ec1 + ex |c2| + |xhat| ec2 + U (|Gr - c1| + |xhat c2| + |Gr - c1 - xhat c2|)) + 2 U |du0| + U |du|.
    At a near-tie element t the mask may differ: Gr_t moves by up to |da_t|, which moves du_t by rstd |da_t| and, through c1 and c2,
    every other element of the plane by rstd |da_t| (1 + |xhat xhat_t|) / N.  dw is continuous there (a_t ~ 0 either way)."""
    u64, w64, dz64 = np.asarray(u, np.float64), np.asarray(w, np.float64), np.asarray(dz, np.float64)
    nb, C, h, wd = u64.shape
    N = h * wd
    xhat, mean, rstd = norm(u64)
    a = np.maximum(xhat, 0.0)
    mask = a > 0
    xmax = np.abs(xhat).max((2, 3), keepdims=True)
    ex = U32 * (rstd * np.abs(mean) + 4.0 * np.maximum(1.0, xmax))
    dw = conv3_wgrad(dz64, a)
    aw = conv3_wgrad(np.abs(dz64), a)
    bw = nb * N * U32 * aw + conv3_wgrad(np.abs(dz64), np.broadcast_to(ex, a.shape)) + U32 * np.abs(dw) + 1e-45
    da = conv3_dgrad(dz64, w64)
    eda = 9 * C * U32 * conv3_dgrad(np.abs(dz64), np.abs(w64)) + U32 * np.abs(da)
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
    ties = np.abs(xhat) < tie
    if ties.any():
        for f, c, y, x in zip(*np.nonzero(ties)):
            jump = rstd[f, c, 0, 0] * abs(da[f, c, y, x])
            bu[f, c] += jump * (1.0 + np.abs(xhat[f, c] * xhat[f, c, y, x])) / N
            bu[f, c, y, x] += jump
    return dw, du, 1.01 * bw, 1.01 * bu, ties
