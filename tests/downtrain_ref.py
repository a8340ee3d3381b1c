"""CPU restatement (numpy, float64) of the backbone's strided stage, Conv2d(Cin -> Cout, 3 x 3, stride 2, pad 1, no bias) ->
InstanceNorm2d(eps 1e-3, no affine) -> ReLU, forward and backward (csrc/down_train.hip).  Pinned to the reference's own autograd by
tests/golden/downtrain_small.npz (tests/test_downtrain_cpu.py); the GPU tests use it where no golden can be stored.

ho = (Hin + 1) // 2, wo = (Win + 1) // 2; z[co, oy, ox] = sum w[co][ci][ky][kx] x[ci, 2 oy + ky - 1, 2 ox + kx - 1] with zero padding;
per plane of z, N = ho wo: mean = sum z / N, rstd = 1 / sqrt(sum z^2 / N - mean^2 + 1e-3), xhat = (z - mean) rstd, h = max(xhat, 0)."""
import numpy as np

from blocktrain_ref import EPS, U32, near_ties, norm, tie_free  # noqa: F401  (applied to z; re-exported for the tests)


def out_size(hin, win):
    return (hin + 1) // 2, (win + 1) // 2


def tap_view(x, ky, kx):
    """v[..., oy, ox] = x[..., 2 oy + ky - 1, 2 ox + kx - 1], zero outside: [.., ho, wo]."""
    ho, wo = out_size(*x.shape[-2:])
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(1, 2), (1, 2)])
    return p[..., ky:ky + 2 * ho - 1:2, kx:kx + 2 * wo - 1:2]


def conv_s2(x, w):
    """x [nb, Cin, Hin, Win], w [Cout, Cin, 3, 3] -> z [nb, Cout, ho, wo], float64."""
    out = 0.0
    for ky in range(3):
        for kx in range(3):
            out = out + np.einsum("oc,nchw->nohw", w[:, :, ky, kx], tap_view(x, ky, kx), optimize=True)
    return out


def conv_s2_wgrad(dz, x):
    """dw[co][ci][ky][kx] = sum_{f, oy, ox} dz[f, co, oy, ox] x[f, ci, 2 oy + ky - 1, 2 ox + kx - 1]."""
    dw = np.empty((dz.shape[1], x.shape[1], 3, 3))
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = np.einsum("nohw,nchw->oc", dz, tap_view(x, ky, kx), optimize=True)
    return dw


def conv_s2_dgrad(dz, w, hin, win):
    """dx[ci, iy, ix] = sum_{co, ky, kx} w[co][ci][ky][kx] dz[co, (iy + 1 - ky) / 2, (ix + 1 - kx) / 2] over whole, in-range quotients."""
    ho, wo = dz.shape[-2:]
    assert (ho, wo) == out_size(hin, win)
    p = np.zeros(dz.shape[:1] + (w.shape[1], hin + 3, win + 3))
    for ky in range(3):
        for kx in range(3):
            p[..., ky:ky + 2 * ho - 1:2, kx:kx + 2 * wo - 1:2] += np.einsum("oc,nohw->nchw", w[:, :, ky, kx], dz, optimize=True)
    return p[..., 1:1 + hin, 1:1 + win]


def down_forward(x, w, return_z=False):
    """h = relu(instance_norm(conv_s2(x, w))) in float64 (and z)."""
    z = conv_s2(np.asarray(x, np.float64), np.asarray(w, np.float64))
    h = np.maximum(norm(z)[0], 0.0)
    return (h, z) if return_z else h


def norm_backward(z, dy):
    """dz = rstd (Gr - mean(Gr) - xhat mean(Gr xhat)), Gr = dy [xhat > 0], float64."""
    xhat, _, rstd = norm(z)
    Gr = np.asarray(dy, np.float64) * (xhat > 0)
    return rstd * (Gr - Gr.mean((2, 3), keepdims=True) - xhat * (Gr * xhat).mean((2, 3), keepdims=True))


def down_backward(x, w, z, dy):
    """x [nb, Cin, Hin, Win], w [Cout, Cin, 3, 3], z, dy [nb, Cout, ho, wo] -> dw [Cout, Cin, 3, 3] summed over the frames,
    dx [nb, Cin, Hin, Win], float64.  z is the conv output the forward stored (the backward normalises it again)."""
    x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    dz = norm_backward(z, dy)
    return conv_s2_wgrad(dz, x64), conv_s2_dgrad(dz, w64, *x64.shape[-2:])


def grad_bounds(x, w, z, dy, tie=1e-5):
    """-> dw, dx (float64), element-wise a-priori bounds bw, bx of |dw32 - dw| and |dx32 - dx| for a float32 implementation working
    from the same float32 inputs, and the near-tie set t = [|xhat64| < tie] of z.  First-order bounds, inflated by 1 % for the
    second-order terms; U = 2^-24.  Derived as blocktrain_ref.grad_bounds:

    xhat32 = fl(fl(z - fl(mean)) fl(rstd)) with mean and rstd from float64 sums:  |xhat32 - xhat| <= ex := U (rstd |mean| +
    4 max(1, max |xhat|)) per plane.
    Gr = dy [xhat > 0] is exact (dy is an input).  c1 = mean(Gr), c2 = mean(Gr xhat32) in float64, rounded once:
        ec1 := U |c1| + s,    ec2 := mean(|Gr| ex) + U |c2| + s |xhat|max,    s := N 2^-53 mean |Gr| for the float64 sums themselves.
    dz = fl(rstd fl(fl(Gr - c1) - fl(xhat c2))):
        e_dz := rstd (ec1 + ex |c2| + |xhat| ec2 + U (|Gr - c1| + |xhat c2| + |Gr - c1 - xhat c2|)) + 2 U |dz|.
    At a near-tie element t the mask may differ: Gr_t moves by |dy_t|, which moves dz_t by rstd |dy_t| and, through c1 and c2, every
    other element of the plane by rstd |dy_t| (1 + |xhat xhat_t|) / N; these jumps are added to e_dz and so reach both products.
    dw sums K_w = nb ho wo products dz32 x in float32 in any order:    |dw err| <= K_w U sum |dz x| + sum e_dz |x| + U |dw|.
    dx sums at most K_x = 4 Cout products w dz32 in any order:        |dx err| <= K_x U sum |w| |dz| + sum |w| e_dz + U |dx|."""
    x64, w64, z64, dy64 = (np.asarray(t, np.float64) for t in (x, w, z, dy))
    nb, cout, ho, wo = z64.shape
    hin, win = x64.shape[-2:]
    N = ho * wo
    xhat, mean, rstd = norm(z64)
    mask = xhat > 0
    xmax = np.abs(xhat).max((2, 3), keepdims=True)
    ex = U32 * (rstd * np.abs(mean) + 4.0 * np.maximum(1.0, xmax))
    Gr = dy64 * mask
    c1 = Gr.mean((2, 3), keepdims=True)
    c2 = (Gr * xhat).mean((2, 3), keepdims=True)
    s = N * 2.0 ** -53 * np.abs(Gr).mean((2, 3), keepdims=True)
    ec1 = U32 * np.abs(c1) + s
    ec2 = (np.abs(Gr) * ex).mean((2, 3), keepdims=True) + U32 * np.abs(c2) + s * xmax
    t3 = Gr - c1 - xhat * c2
    dz = rstd * t3
    e_dz = rstd * (ec1 + ex * np.abs(c2) + np.abs(xhat) * ec2 + U32 * (np.abs(Gr - c1) + np.abs(xhat * c2) + np.abs(t3))) + 2 * U32 * np.abs(dz)
    ties = np.abs(xhat) < tie
    if ties.any():
        for f, c, y, xx in zip(*np.nonzero(ties)):
            jump = rstd[f, c, 0, 0] * abs(dy64[f, c, y, xx])
            e_dz[f, c] += jump * (1.0 + np.abs(xhat[f, c] * xhat[f, c, y, xx])) / N
            e_dz[f, c, y, xx] += jump
    ax, aw = np.abs(x64), np.abs(w64)
    dw = conv_s2_wgrad(dz, x64)
    bw = nb * N * U32 * conv_s2_wgrad(np.abs(dz), ax) + conv_s2_wgrad(e_dz, ax) + U32 * np.abs(dw) + 1e-45
    dx = conv_s2_dgrad(dz, w64, hin, win)
    bx = 4 * cout * U32 * conv_s2_dgrad(np.abs(dz), aw, hin, win) + conv_s2_dgrad(e_dz, aw, hin, win) + U32 * np.abs(dx) + 1e-45
    return dw, dx, 1.01 * bw, 1.01 * bx, ties
