"""CPU restatement (numpy, float64) of the loss gradient (csrc/train.hip: k_loss_grad) and of the anchor head with its layout
permutation, forward and backward (k_head_dw / k_head_dx).  Pinned to the reference's own autograd by tests/golden/headtrain_small.npz
and lossgrad_eight_20cm.npz (tests/test_headtrain_cpu.py); the GPU tests use it where no golden can be stored (full-size head)."""
import numpy as np

LOC_WEIGHT, CLS_WEIGHT, DIR_WEIGHT = 0.25, 1.0, 0.2
HEAD_KEYS = ("heads.conv_cls.weight", "heads.conv_cls.bias", "heads.conv_box.weight", "heads.conv_box.bias",
             "heads.conv_dir.weight", "heads.conv_dir.bias")


def loss_grad(cls, box, dr, labels, tgt, dirt, grad_scale=1.0, batch_div=None):
    """d loss / d (cls [nb,A], box [nb,A,7], dr [nb,A,2]) of LossGenerator.generate's `loss` (NormByNumPositives, weights
    0.25 / 1.0 / 0.2, 1 / batch mean), float64."""
    cls = np.asarray(cls, np.float64).reshape(labels.shape)
    nb, A = labels.shape
    box = np.asarray(box, np.float64).reshape(nb, A, 7)
    dr = np.asarray(dr, np.float64).reshape(nb, A, 2)
    tgt = np.asarray(tgt, np.float64).reshape(nb, A, 7)
    dirt = np.asarray(dirt).reshape(nb, A)
    pos = labels > 0
    inv = grad_scale / (nb if batch_div is None else batch_div) / np.maximum(pos.sum(1, keepdims=True), 1)
    # focal: z = -x for positives, x for negatives; 1 - p_t = sigmoid(z), cross entropy = softplus(z)
    z = np.where(pos, -cls, cls)
    e = np.exp(-np.abs(z))
    sig = np.where(z >= 0, 1.0, e) / (1.0 + e)
    om = np.where(z >= 0, e, 1.0) / (1.0 + e)
    sp = np.maximum(z, 0.0) + np.log1p(e)
    g = np.where(pos, 0.25, 0.75) * sig * sig * (2.0 * om * sp + sig)
    dcls = np.where(pos, -g, g) * (labels >= 0) * inv * CLS_WEIGHT
    # smooth L1 (sigma 3) with the sin difference on code 6
    d = box - tgt
    d[..., 6] = np.sin(box[..., 6]) * np.cos(tgt[..., 6]) - np.cos(box[..., 6]) * np.sin(tgt[..., 6])
    gl = np.where(np.abs(d) <= 1.0 / 9.0, 9.0 * d, np.sign(d))
    gl[..., 6] *= np.cos(box[..., 6]) * np.cos(tgt[..., 6]) + np.sin(box[..., 6]) * np.sin(tgt[..., 6])
    dbox = gl * (pos * inv)[..., None] * LOC_WEIGHT
    # 2-way softmax cross entropy: softmax - onehot
    dd = dr[..., 1] - dr[..., 0]
    e = np.exp(-np.abs(dd))
    p1 = np.where(dd >= 0, 1.0, e) / (1.0 + e)
    p0 = np.where(dd >= 0, e, 1.0) / (1.0 + e)
    g0 = np.where(dirt > 0, p0, -p1)
    ddir = np.stack([g0, -g0], -1) * (pos * inv)[..., None] * DIR_WEIGHT
    return dcls, dbox, ddir


def natural_weights(sd, dtype=np.float64):
    """state_dict -> W [10 na, 320], b [10 na]: rows cls a | box a * 7 + k | dir a * 2 + k (state_dict order, concatenated)."""
    W = np.concatenate([np.asarray(sd[k], dtype).reshape(-1, 320) for k in HEAD_KEYS[0::2]])
    b = np.concatenate([np.asarray(sd[k], dtype).reshape(-1) for k in HEAD_KEYS[1::2]])
    return W, b


def split_rows(M, na):
    """[10 na, ...] in natural row order -> the (cls, box, dir) blocks."""
    return M[:na], M[na:8 * na], M[8 * na:]


def rows_to_outputs(Y, na, H, W):
    """Y [nb, 10 na, H, W] channel-major -> the head's output layout: cls [nb, A, 1], box [nb, A, 7], dir [nb, A, 2], ordered
    (anchor type, x, y) with the codes innermost (SharedHead.forward's view / permute)."""
    nb = Y.shape[0]
    c, b, d = Y[:, :na], Y[:, na:8 * na], Y[:, 8 * na:]
    return (c.reshape(nb, -1, 1), b.reshape(nb, na, 7, H, W).transpose(0, 1, 3, 4, 2).reshape(nb, -1, 7),
            d.reshape(nb, na, 2, H, W).transpose(0, 1, 3, 4, 2).reshape(nb, -1, 2))


def outputs_to_rows(cls, box, dr, na, H, W):
    """Inverse of rows_to_outputs: gradients in the output layout -> dY [nb, 10 na, H * W]."""
    nb = box.shape[0]
    c = np.asarray(cls).reshape(nb, na, H * W)
    b = np.asarray(box).reshape(nb, na, H, W, 7).transpose(0, 1, 4, 2, 3).reshape(nb, 7 * na, H * W)
    d = np.asarray(dr).reshape(nb, na, H, W, 2).transpose(0, 1, 4, 2, 3).reshape(nb, 2 * na, H * W)
    return np.concatenate([c, b, d], 1)


def head_forward(x, W, b, na):
    nb, _, H, Wd = x.shape
    Y = np.einsum("rc,ncp->nrp", W, x.reshape(nb, 320, -1)) + b[None, :, None]
    return rows_to_outputs(Y.reshape(nb, -1, H, Wd), na, H, Wd)


def head_backward(x, dcls, dbox, ddir, W, na, bounds=False):
    """x [nb,320,H,W], output-layout gradients, W [10 na, 320] -> dW [10 na, 320], db [10 na], dx [nb,320,H,W] in float64.
    bounds=True adds the sums of |a_k b_k| of each result element (for the a-priori float32 summation bounds)."""
    nb, _, H, Wd = x.shape
    X = np.asarray(x, np.float64).reshape(nb, 320, -1)
    dY = outputs_to_rows(np.asarray(dcls, np.float64), np.asarray(dbox, np.float64), np.asarray(ddir, np.float64), na, H, Wd)
    W = np.asarray(W, np.float64)
    XT = X.transpose(0, 2, 1)
    dW = np.matmul(dY, XT).sum(0)
    db = dY.sum((0, 2))
    dx = np.matmul(W.T[None], dY).reshape(x.shape)
    if not bounds:
        return dW, db, dx
    return dW, db, dx, (np.matmul(np.abs(dY), np.abs(XT)).sum(0), np.abs(dY).sum((0, 2)),
                        np.matmul(np.abs(W).T[None], np.abs(dY)).reshape(x.shape))


def sum_bound(K, abs_sum, value):
    """A-priori bound of a float32 sum of K products in any order, K * 2^-24 * sum |a_k b_k|, plus one float32 rounding of the result."""
    return K * 2.0 ** -24 * abs_sum + 2.0 ** -24 * np.abs(value) + 1e-45
