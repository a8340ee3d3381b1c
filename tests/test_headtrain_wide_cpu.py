"""CPU: the float64 restatement of the anchor head (tests/headtrain_ref.py) at more than 9 anchors per location, against torch's own
float64 autograd of F.conv2d with the concatenated [10 na, 320, 1, 1] weight.  The reference has no head with more than 9 anchors
and so no golden; this pins head_forward, head_backward and the layout permutation (rows_to_outputs / outputs_to_rows) at na = 10,
20 and 24 independently of the device code, before tests/test_headtrain_wide_gpu.py judges that code by them.  One map with H != W,
two frames."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import headtrain_ref as R

NB, H, W = 2, 5, 3


@pytest.mark.parametrize("na", [10, 20, 24])
def test_ref_against_torch_autograd(na):
    rng = np.random.default_rng(na)
    rows = 10 * na
    x = rng.standard_normal((NB, 320, H, W))
    Wn = rng.standard_normal((rows, 320)) * 0.05
    bn = rng.standard_normal(rows)
    xt = torch.from_numpy(x).requires_grad_(True)
    wt = torch.from_numpy(Wn.reshape(rows, 320, 1, 1).copy()).requires_grad_(True)
    bt = torch.from_numpy(bn.copy()).requires_grad_(True)
    Y = F.conv2d(xt, wt, bt)
    assert Y.dtype == torch.float64 and Y.shape == (NB, rows, H, W)
    # forward: the restatement's outputs are torch's channels in the head's output layout
    got = R.head_forward(x, Wn, bn, na)
    want = R.rows_to_outputs(Y.detach().numpy(), na, H, W)
    for g, w, codes in zip(got, want, (1, 7, 2)):
        assert g.shape == w.shape == (NB, na * H * W, codes)
        np.testing.assert_allclose(g, w, rtol=1e-12, atol=1e-12 * np.abs(w).max())  # (an element may cancel: 320 terms in another order)
    # the layout itself, spelled out once more: anchor a, code k of box is channel na + 7 a + k, of dir 8 na + 2 a + k
    Yn = Y.detach().numpy()
    a, k, h, w_ = na - 1, 5, H - 1, 1
    assert want[1][1, (a * H + h) * W + w_, k] == Yn[1, na + 7 * a + k, h, w_]
    assert want[2][0, (a * H + h) * W + w_, 1] == Yn[0, 8 * na + 2 * a + 1, h, w_]
    assert want[0][1, (a * H + h) * W + w_, 0] == Yn[1, a, h, w_]
    # backward: upstream gradients in the output layout
    dcls, dbox, ddir = (rng.standard_normal(t.shape) for t in want)
    # SharedHead.forward's view / permute on the torch tensor, so that autograd carries them back to the channels
    c = Y[:, :na].reshape(NB, -1, 1)
    b = Y[:, na:8 * na].reshape(NB, na, 7, H, W).permute(0, 1, 3, 4, 2).reshape(NB, -1, 7)
    d = Y[:, 8 * na:].reshape(NB, na, 2, H, W).permute(0, 1, 3, 4, 2).reshape(NB, -1, 2)
    assert all(np.array_equal(t.detach().numpy(), w) for t, w in zip((c, b, d), want))
    ((c * torch.from_numpy(dcls)).sum() + (b * torch.from_numpy(dbox)).sum() + (d * torch.from_numpy(ddir)).sum()).backward()
    dW, db, dx = R.head_backward(x, dcls, dbox, ddir, Wn, na)
    np.testing.assert_allclose(dW, wt.grad.numpy().reshape(rows, 320), rtol=1e-12, atol=1e-12 * np.abs(dW).max())
    np.testing.assert_allclose(db, bt.grad.numpy(), rtol=1e-12, atol=1e-12 * np.abs(db).max())
    np.testing.assert_allclose(dx, xt.grad.numpy(), rtol=1e-12, atol=1e-12 * np.abs(dx).max())
    # and the bounds' sums are those of the absolute values
    _, _, _, (aW, ab, ax) = R.head_backward(x, dcls, dbox, ddir, Wn, na, bounds=True)
    assert (aW >= np.abs(dW) * (1 - 1e-12)).all() and (ab >= np.abs(db) * (1 - 1e-12)).all() and (ax >= np.abs(dx) * (1 - 1e-12)).all()
