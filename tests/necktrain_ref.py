"""CPU restatement (numpy, float64) of one upsampling branch of RPN, ConvTranspose2d(k = s, no bias) -> InstanceNorm2d(eps 1e-3, no
affine) -> ReLU, forward and backward (csrc/neck_train.hip).  Pinned to the reference's own autograd by
tests/golden/necktrain_small.npz (tests/test_necktrain_cpu.py); the GPU tests use it where no golden can be stored.

A ConvTranspose with kernel = stride is a GEMM on the input grid: rows r = co s s + ky s + kx, Z[r][q] = sum_ci w[ci][r] x[ci][q] is
output element (co, s qy + ky, s qx + kx)."""
import numpy as np

EPS = 1e-3
CIN = (64, 128, 256)
CUP = (64, 128, 128)
COFF = (0, 64, 192)
KEYS = ("rpn.deconv1.0.weight", "rpn.deconv2.0.weight", "rpn.deconv3.0.weight")


def to_rows(t, s):
    """[nb, C, s h, s w] -> the GEMM layout [nb, C s s, h w]."""
    nb, C, H, W = t.shape
    h, w = H // s, W // s
    return t.reshape(nb, C, h, s, w, s).transpose(0, 1, 3, 5, 2, 4).reshape(nb, C * s * s, h * w)


def from_rows(t, s, h, w):
    nb, R, _ = t.shape
    C = R // (s * s)
    return t.reshape(nb, C, s, s, h, w).transpose(0, 1, 4, 2, 5, 3).reshape(nb, C, h * s, w * s)


def conv_t(x, w):
    """x [nb, Cin, h, w], w [Cin, Cup, s, s] -> [nb, Cup, s h, s w], float64."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    nb, cin, h, wd = x.shape
    s = w.shape[2]
    Z = np.matmul(w.reshape(cin, -1).T[None], x.reshape(nb, cin, -1))
    return from_rows(Z, s, h, wd)


def norm_stats(Z):
    mean = Z.mean((2, 3), keepdims=True)
    rstd = 1.0 / np.sqrt(Z.var((2, 3), keepdims=True) + EPS)
    return mean, rstd


def branch_forward(x, w, return_xhat=False):
    """relu(instance_norm(conv_t(x, w))) in float64 (and xhat)."""
    Z = conv_t(x, w)
    mean, rstd = norm_stats(Z)
    xhat = (Z - mean) * rstd
    y = np.maximum(xhat, 0.0)
    return (y, xhat) if return_xhat else y


def branch_backward(x, w, y, dy, bounds=False):
    """x [nb, Cin, h, w], w [Cin, Cup, s, s], y / dy [nb, Cup, s h, s w] (the branch's channel slice of rpn_out and of its gradient; the
    ReLU mask is taken from the GIVEN y) -> dw [Cin, Cup, s, s], dx [nb, Cin, h, w] in float64.  bounds=True adds the sums of
    |a_k b_k| of each element of dw and dx (for the a-priori float32 summation bounds)."""
    x64 = np.asarray(x, np.float64)
    w64 = np.asarray(w, np.float64)
    nb, cin, h, wd = x64.shape
    s = w64.shape[2]
    Z = conv_t(x64, w64)
    mean, rstd = norm_stats(Z)
    xhat = (Z - mean) * rstd
    Gr = np.asarray(dy, np.float64) * (np.asarray(y) > 0)
    dZ = rstd * (Gr - Gr.mean((2, 3), keepdims=True) - xhat * (Gr * xhat).mean((2, 3), keepdims=True))
    dZr = to_rows(dZ, s)                                  # [nb, R, p]
    X = x64.reshape(nb, cin, -1)                          # [nb, Cin, p]
    Wr = w64.reshape(cin, -1)                             # [Cin, R]
    dw = np.matmul(X, dZr.transpose(0, 2, 1)).sum(0).reshape(w64.shape)
    dx = np.matmul(Wr[None], dZr).reshape(x64.shape)
    if not bounds:
        return dw, dx
    aw = np.matmul(np.abs(X), np.abs(dZr).transpose(0, 2, 1)).sum(0).reshape(w64.shape)
    ax = np.matmul(np.abs(Wr)[None], np.abs(dZr)).reshape(x64.shape)
    return dw, dx, (aw, ax), dict(Z=Z, rstd=rstd, Gr=Gr, xhat=xhat)


def sum_bound(K, abs_sum, value):
    """A-priori bound of a float32 sum of K products in any order, K * 2^-24 * sum |a_k b_k|, plus one float32 rounding of the result
    (headtrain_ref.sum_bound)."""
    return K * 2.0 ** -24 * abs_sum + 2.0 ** -24 * np.abs(value) + 1e-45


def grad_bounds(x, w, y, dy):
    """Element-wise a-priori bounds of |dw32 - dw64| and |dx32 - dx64| for a float32 implementation that recomputes Z, its statistics
    and dZ in float32 from the same float32 inputs, and the float64 results.

    With u = 2^-24: Z is a float32 sum of Cin products, |Z32 - Z| <= (Cin + 2) u sum |w x|; the statistics are float64 sums of those
    Z32, so mean and rstd inherit at most that error, and xhat32 = (Z32 - mean) rstd adds a few roundings:
        d_xhat <= ez := u ((Cin + 2) 2 max(sum |w x|) rstd + 8 max(1, max |xhat|))        per frame and channel.
    dZ = rstd ((Gr - c1) - xhat c2) with c1 = mean(Gr), c2 = mean(Gr xhat), |c1| <= max |Gr|, |c2| <= max |Gr| max |xhat|; its
    float32 evaluation from xhat32 (c2 inherits d_xhat max |Gr|, rstd a relative error below ez) is off by at most
        E := ez rstd max |Gr| (1 + 3 max |xhat|)                                           per element of the channel.
    Every dZ element perturbed by E, then summed in float32 in any order:
        |dw err| <= K_w u sum |x dZ| + sum |x| E,      K_w = nb h w
        |dx err| <= K_x u sum |w dZ| + sum |w| E,      K_x = Cup s s
    plus one rounding of the result."""
    dw, dx, (aw, ax), t = branch_backward(x, w, y, dy, bounds=True)
    x64 = np.abs(np.asarray(x, np.float64))
    w64 = np.abs(np.asarray(w, np.float64))
    nb, cin, h, wd = x64.shape
    s = w64.shape[2]
    xmax = np.abs(t["xhat"]).max((2, 3), keepdims=True)
    absz = conv_t(x64, w64).max((2, 3), keepdims=True)
    ez = 2.0 ** -24 * ((cin + 2) * 2.0 * absz * t["rstd"] + 8.0 * np.maximum(1.0, xmax))
    gmax = np.abs(t["Gr"]).max((2, 3), keepdims=True)
    E = ez * t["rstd"] * gmax * (1.0 + 3.0 * xmax)                                            # [nb, Cup, 1, 1]
    Er = to_rows(np.broadcast_to(E, t["Z"].shape), s)                                          # [nb, R, p]
    X = x64.reshape(nb, cin, -1)
    ew = np.matmul(X, Er.transpose(0, 2, 1)).sum(0).reshape(w64.shape)
    ex = np.matmul(w64.reshape(cin, -1)[None], Er).reshape(x64.shape)
    bw = sum_bound(nb * h * wd, aw, dw) + ew
    bx = sum_bound(w64.shape[1] * s * s, ax, dx) + ex
    return dw, dx, bw, bx
