"""Float64 restatement of the pillar feature net in train mode (reference networks/pointpillars8_shared.py:11-60: decoration, Conv1d(9 -> 64,
no bias), BatchNorm1d with batch statistics, ReLU, max over the T slots) and of its backward in the closed form csrc/pfn_train.hip
evaluates.  tests/golden/make_pfntrain_goldens.py asserts it against the reference's float64 autograd before it writes the fixture.

Notation: f[p,t,0:9] the decorated features, zero for padded slots t >= n_p; N = P T counts every slot, as BatchNorm1d does.
    s[k] = sum f[.,.,k],  M[j,k] = sum f[.,.,j] f[.,.,k],  z = f W^T,  mean_c = W_c s / N,  var_c = W_c M W_c^T / N - mean_c^2,
    y = gamma (z - mean) invstd + beta,  feat = max_t relu(y),  arg = the first slot that attains it (n_p when a padded slot wins).
Backward from g = dL/dfeat (zeroed where feat <= 0), t* = arg, zhat* = (z[p,t*,c] - mean_c) invstd_c:
    S1 = sum_p g,  S2 = sum_p g zhat*,  G[c,k] = sum_p g f[p,t*,k],  dbeta = S1,  dgamma = S2,
    dW[c,k] = gamma_c invstd_c (G[c,k] - S1_c s_k / N - S2_c invstd_c ((W M)[c,k] - mean_c s_k) / N)."""
import numpy as np

EPS = 1e-5
MOMENTUM = 0.1
F64 = np.float64


def features(voxels, coors, npts, vx, vy, x_off, y_off):
    """f64[P,T,9].  The cell centre is float32 arithmetic in the reference whatever the dtype of the run (coors.float() * vx + x_offset
    with float32 scalars); everything else is float64 here."""
    v = np.asarray(voxels, F64)
    P, T, _ = v.shape
    n = np.asarray(npts).astype(np.int64)
    mean = v[:, :, :3].sum(1, keepdims=True) / n.astype(F64).reshape(-1, 1, 1)
    c32 = np.asarray(coors)[:, :2].astype(np.float32)
    cx = (c32[:, 0] * np.float32(vx) + np.float32(x_off)).astype(F64)
    cy = (c32[:, 1] * np.float32(vy) + np.float32(y_off)).astype(F64)
    f = np.concatenate([v, v[:, :, :3] - mean, v[:, :, :1] - cx[:, None, None], v[:, :, 1:2] - cy[:, None, None]], -1)
    return f * (np.arange(T)[None, :] < n[:, None])[:, :, None]


def forward(f, w, gamma, beta):
    """-> dict(N, s, M, mean, var (biased), invstd, z [P,T,64], y, feat [P,64], arg [P,64] uint8)."""
    W = np.asarray(w, F64).reshape(64, 9)
    gamma, beta = np.asarray(gamma, F64), np.asarray(beta, F64)
    P, T, _ = f.shape
    N = P * T
    s = f.sum((0, 1))
    M = np.einsum("ptj,ptk->jk", f, f)
    mean = W @ s / N
    var = np.einsum("cj,jk,ck->c", W, M, W) / N - mean ** 2
    invstd = 1.0 / np.sqrt(var + EPS)
    z = f @ W.T
    y = gamma * (z - mean) * invstd + beta
    a = np.maximum(y, 0.0)
    arg = a.argmax(1)  # the first maximiser; every padded slot carries the same value, so the first of them is slot n_p
    return dict(N=N, s=s, M=M, mean=mean, var=var, invstd=invstd, z=z, y=y, feat=a.max(1), arg=arg.astype(np.uint8))


def running(rm, rv, fwd):
    """BatchNorm1d's update of the running statistics (momentum 0.1, unbiased variance)."""
    N = fwd["N"]
    return (1 - MOMENTUM) * np.asarray(rm, F64) + MOMENTUM * fwd["mean"], (1 - MOMENTUM) * np.asarray(rv, F64) + MOMENTUM * fwd["var"] * N / (N - 1)


def backward(f, w, gamma, fwd, g, arg=None):
    """-> (dW [64,9], dgamma [64], dbeta [64]) by the closed form; arg: evaluate at a given selection instead of the forward's."""
    W = np.asarray(w, F64).reshape(64, 9)
    gamma = np.asarray(gamma, F64)
    N, s, M, mean, invstd = fwd["N"], fwd["s"], fwd["M"], fwd["mean"], fwd["invstd"]
    arg = (fwd["arg"] if arg is None else np.asarray(arg)).astype(np.int64)
    P = f.shape[0]
    g = np.where(fwd["feat"] > 0, np.asarray(g, F64), 0.0)
    fs = f[np.arange(P)[:, None], arg]                      # [P,64,9]
    zs = np.take_along_axis(fwd["z"], arg[:, None, :], 1)[:, 0]  # [P,64]
    zh = (zs - mean) * invstd
    S1, S2 = g.sum(0), (g * zh).sum(0)
    G = np.einsum("pc,pck->ck", g, fs)
    dW = (gamma * invstd)[:, None] * (G - S1[:, None] * s[None] / N - (S2 * invstd)[:, None] * (W @ M - mean[:, None] * s[None]) / N)
    return dW, S2, S1


def margins(y, npts):
    """Over every (p, c): the smallest gap between the two largest candidates (the real slots plus one padded slot) and the smallest
    |largest candidate|, from the pre-ReLU activations y [P,T,64]."""
    P, T, _ = y.shape
    n = np.asarray(npts).astype(np.int64)
    cand = np.where((np.arange(T)[None, :] <= n[:, None])[:, :, None], y, -np.inf)  # slot n_p (if any) is the padded candidate
    top = np.sort(cand, 1)[:, -2:]
    gap = np.where(np.isfinite(top[:, 0]), top[:, 1] - top[:, 0], np.inf)
    return float(gap.min()), float(np.abs(top[:, 1]).min())


def maximiser_slack(y, arg):
    """How far below the maximum of relu(y) over the slots each given arg lies, [P,64] (0 for a true maximiser)."""
    a = np.maximum(y, 0.0)
    return a.max(1) - np.take_along_axis(a, np.asarray(arg).astype(np.int64)[:, None, :], 1)[:, 0]
