"""CPU restatement (numpy, float64) of the whole RPN, forward and backward: per level the strided stage (downtrain_ref), the Resnet
modules (blocktrain_ref) and the upsampling branch (necktrain_ref), wired by the same table as the network's _RpnFunction.  Pinned to
the reference's own autograd by tests/golden/rpntrain_small.npz (tests/test_rpntrain_cpu.py): that is what checks the wiring -- the
residual adds, the unit order and where an upsampler's dx joins the gradient of a block output.

Level b (C = 64, 128, 256): h = relu(norm(conv_s2(x_{b-1}, w_down))); a module of two convolutions maps r -> r + U(U(r, w_i), w_{i+1}),
one of a single convolution r -> r + U(r, w_i), with U(u, w) = conv3(relu(norm(u)), w); x_b is the last module's output and
y_b = relu(norm(conv_t(x_b, w_up))) its slice of rpn_out."""
import numpy as np

import blocktrain_ref as B
import downtrain_ref as D
import necktrain_ref as N

# (level, convolutions per Resnet module in forward order)
RPN_TABLE = ((0, (2, 1)), (1, (2, 2, 1)), (2, (2, 2, 1)))
W0 = (0, 4, 10)  # a level's strided convolution among the sixteen; its unit convolutions follow
UNITS = ("3.conv_block.2", "3.conv_block.5", "4.conv_block.2", "4.conv_block.5", "5.conv_block.2")
CONV_KEYS = tuple(f"rpn.block{b + 1}.{k}.weight" for b, mods in RPN_TABLE for k in ("0",) + UNITS[:sum(mods)])
NECK_KEYS = N.KEYS
# the nineteen weights in the reference's state_dict order: a block's convolutions, then its upsampler
KEYS = tuple(k for b in range(3) for k in CONV_KEYS[W0[b]:W0[b] + 1 + sum(RPN_TABLE[b][1])] + (NECK_KEYS[b],))


def rpn_forward(canvas, wc, wn):
    """canvas [nb,64,gx,gy], wc the sixteen convolutions in CONV_KEYS order, wn the three upsamplers -> dict: y [nb,320,H,W], taps
    (x1, x2, x3), units (per level the unit inputs, unit order), zs (per level the strided convolution's raw output), float64."""
    x = np.asarray(canvas, np.float64)
    taps, units, zs, ys = [], [], [], []
    for b, mods in RPN_TABLE:
        w = [np.asarray(t, np.float64) for t in wc[W0[b]:W0[b] + 1 + sum(mods)]]
        r, z = D.down_forward(x, w[0], return_z=True)
        us, i = [], 1
        for n in mods:
            us.append(r)
            if n == 2:
                us.append(B.unit_forward(r, w[i]))
                r = r + B.unit_forward(us[-1], w[i + 1])
            else:
                r = r + B.unit_forward(r, w[i])
            i += n
        x = r
        taps.append(x), units.append(us), zs.append(z)
        ys.append(N.branch_forward(x, wn[b]))
    return dict(y=np.concatenate(ys, 1), taps=taps, units=units, zs=zs)


def relu_masks(y, units, zs):
    """The branch every ReLU takes, from the tensors a forward hands out (float64 here, the GPU's float32 taps in the GPU test): per
    level the stage's [xhat(z) > 0], each unit's [xhat(u) > 0] and the upsampler's [y > 0] -> {site name: bool array}."""
    out = {}
    for b in range(3):
        out[f"stage{b}"] = B.norm(zs[b])[0] > 0
        for k, u in enumerate(units[b]):
            out[f"unit{b}.{k}"] = B.norm(u)[0] > 0
        out[f"up{b}"] = np.asarray(y)[:, N.COFF[b]:N.COFF[b] + N.CUP[b]] > 0
    return out


def block_backward(mods, units, weights, g):
    """_RpnFunction's rpn_block_backward in float64: -> (dw per unit, dL/d(block input h))."""
    dws = [None] * len(units)
    i = len(units)
    for n in reversed(mods):
        i -= n
        if n == 2:
            dws[i + 1], gm = B.unit_backward(units[i + 1], weights[i + 1], g)
            dws[i], g = B.unit_backward(units[i], weights[i], gm, dskip=g)
        else:
            dws[i], g = B.unit_backward(units[i], weights[i], g, dskip=g)
    return dws, g


def rpn_backward(canvas, wc, wn, fwd, dy):
    """-> (dwc: sixteen, dwn: three, dcanvas), float64, from a forward's tensors `fwd` (rpn_forward's dict) and dy [nb,320,H,W]."""
    y, taps, units, zs = fwd["y"], fwd["taps"], fwd["units"], fwd["zs"]
    dwn, dxn = [], []
    for b in range(3):
        sl = slice(N.COFF[b], N.COFF[b] + N.CUP[b])
        dw, dx = N.branch_backward(taps[b], wn[b], y[:, sl], np.asarray(dy)[:, sl])
        dwn.append(dw), dxn.append(dx)
    dwc = [None] * 16
    g = None
    for b, mods in reversed(RPN_TABLE):
        n, w0 = sum(mods), W0[b]
        g = dxn[b] if g is None else dxn[b] + g
        dwc[w0 + 1:w0 + 1 + n], gh = block_backward(mods, units[b], wc[w0 + 1:w0 + 1 + n], g)
        dwc[w0], g = D.down_backward(canvas if b == 0 else taps[b - 1], wc[w0], zs[b], gh)
    return dwc, dwn, g
