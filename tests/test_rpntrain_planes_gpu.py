"""GPU tests of pp_unit_backward and pp_down_backward on planes of more than 16384 elements, where the streaming passes (statistics,
pack, norm backward, parity planes) cut a plane into several segments: what levels 0 and 1 of the workload run and no smaller test
reaches.  Sizes: the smallest at which a tight plane (N elements, S segments) and its padded plane (PS elements, SP slices) split, with
N and PS no multiples of 256 (the last segment is clamped), S != SP in two of the four cases, and segments longer than 1024 elements (the
four-way unrolled loop).

  unit 64 x 150 x 131, 2 frames   N = 19650  S = 2   PS = 20520  SP = 2
  unit 64 x 128 x 127, 1 frame    N = 16256  S = 1   PS = 17068  SP = 2
  down 64 -> 64  from 301 x 263, 2 frames   N = 19932  S = 2   PS = 20808  SP = 2
  down 64 -> 64  from 255 x 253, 1 frame    N = 16256  S = 1   PS = 17068  SP = 2

Every gradient is held to the a-priori float32 bound of blocktrain_ref / downtrain_ref.grad_bounds against the float64 restatement; a
frame alone gives the bits it gives inside a batch, and a repeated call gives the same bits."""
import numpy as np
import pytest
import torch

import blocktrain_ref as RB
import downtrain_ref as RD
from train_common import check_bound, dev, engine
from train_common import random_case as unit_case
from test_downtrain_gpu import random_case as down_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("C,h,w,nb", [(64, 150, 131, 2), (64, 128, 127, 1)])
def test_unit_backward_segmented_planes(C, h, w, nb):
    eng = engine()
    u, wt, dz, dskip = unit_case(C, h, w, nb, 300 + h)
    assert (h + 2) * (w + 2) > 16384
    ud, wd, dzd, dsd = dev(u), dev(wt), dev(dz), dev(dskip)
    dw, du = eng.unit_backward(ud, wd, dzd, dskip=dsd)
    rw, ru, bw, bu, ties = RB.grad_bounds(u, wt, dz, dskip=dskip)
    assert not ties.any()
    what = f"unit {C}x{h}x{w}x{nb}"
    check_bound(dw, rw, bw, what + " dw")
    check_bound(du, ru, bu, what + " du")
    dw2, du2 = eng.unit_backward(ud, wd, dzd, dskip=dsd)
    assert torch.equal(dw, dw2) and torch.equal(du, du2)
    for f in range(nb if nb > 1 else 0):
        s = slice(f, f + 1)
        _, duf = eng.unit_backward(ud[s], wd, dzd[s], dskip=dsd[s])
        assert torch.equal(duf[0], du[f]), f  # a frame's du does not depend on the batch it rides in


@pytest.mark.parametrize("cin,cout,hin,win,nb", [(64, 64, 301, 263, 2), (64, 64, 255, 253, 1)])
def test_down_backward_segmented_planes(cin, cout, hin, win, nb):
    eng = engine()
    x, w, z, dy = down_case(cin, cout, hin, win, nb, 300 + hin)
    assert z.shape[2] * z.shape[3] > 16000 and (z.shape[2] + 2) * (z.shape[3] + 2) > 16384
    xd, wd, zd, dyd = dev(x), dev(w), dev(z), dev(dy)
    dw, dx = eng.down_backward(xd, wd, zd, dyd)
    rw, rx, bw, bx, ties = RD.grad_bounds(x, w, z, dy)
    assert not ties.any()
    what = f"down {cin}->{cout} {hin}x{win}x{nb}"
    check_bound(dw, rw, bw, what + " dw")
    check_bound(dx, rx, bx, what + " dx")
    dw2, dx2 = eng.down_backward(xd, wd, zd, dyd)
    dw3, none = eng.down_backward(xd, wd, zd, dyd, need_dx=False)
    assert none is None and torch.equal(dw, dw2) and torch.equal(dx, dx2) and torch.equal(dw, dw3)
    for f in range(nb if nb > 1 else 0):
        s = slice(f, f + 1)
        _, dxf = eng.down_backward(xd[s], wd, zd[s], dyd[s])
        assert torch.equal(dxf[0], dx[f]), f  # a frame's dx does not depend on the batch it rides in
