"""CPU: the backward walk of the RPN, pinned call by call.  The three autograd Functions of networks/pointpillars8_shared.py run one
forward and backward on CPU tensors with the stand-in engine of tests/golden/make_rpnwalk_trace.py, which records every engine call
with the tensor that went into each argument; the traces must equal tests/golden/rpn_walk_trace.json, recorded once from the code in
front of the refactor that gave the three norm forms one walk (that file says why it is not recorded again).  And the door of Engine
itself: the *_affine / *_bn methods and the norm= form hand the library the same entry and the same arguments."""
import json
import sys

import pytest
import torch

from conftest import GOLDEN, load_pkg

sys.path.insert(0, GOLDEN)
import make_rpnwalk_trace as G  # noqa: E402

with open(G.PATH) as _f:
    TRACE = json.load(_f)


def test_the_golden_holds_exactly_the_cases():
    assert list(TRACE) == [G.case_name(c) for c in G.cases()]
    for first, calls in zip(G.FIRSTS, (21, 11, 10, 5)):  # the call plan of a full step at each depth, taps included
        assert len(TRACE[f"instance first={first} all fp32/fp32"]["calls"]) == calls


@pytest.mark.parametrize("case", G.cases(), ids=G.case_name)
def test_walk_makes_the_recorded_calls(case):
    got = G.run_case(load_pkg("networks.pointpillars8_shared"), case)
    want = TRACE[G.case_name(case)]
    assert got["calls"] == want["calls"]
    assert got["grads"] == want["grads"]


def door_engine(engine, monkeypatch, inputs=()):
    """An Engine without a device or a library.  _call_backward records (entry, arguments): an input tensor by its name in `inputs`,
    a tensor the method allocated by dtype and shape."""
    monkeypatch.setattr(engine, "_chk", lambda t, dtype, shape, what: t)  # it wants CUDA tensors
    eng = object.__new__(engine.Engine)
    eng.max_batch, eng.H, eng.W, eng.device, eng.log = 4, 8, 4, torch.device("cpu"), []
    names = {t.data_ptr(): n for n, t in inputs}
    seen = lambda a: names.get(a.data_ptr(), (str(a.dtype), tuple(a.shape))) if isinstance(a, torch.Tensor) else a  # noqa: E731
    eng._call_backward = lambda entry, *args: eng.log.append((entry, [seen(a) for a in args]))
    return eng


@pytest.mark.parametrize("family", ("unit", "down", "neck"))
@pytest.mark.parametrize("form", ("affine", "bn"))
def test_engine_door_forms_agree(family, form, monkeypatch):
    """The nine-method convention and norm= reach _call_backward with the same entry name and argument list, flags included."""
    engine = load_pkg("engine")
    nb, c = 2, 64
    shapes = {"x": (nb, c, 8, 4), "dx": (nb, c, 8, 4), "skip": (nb, c, 8, 4), "w": (c, c, 3, 3), "wn": (c, c, 1, 1), "z": (nb, c, 4, 2),
              "dz": (nb, c, 4, 2), "y": (nb, 320, 8, 4), "dy": (nb, 320, 8, 4), "scale": (c,), "shift": (c,), "mean": (c,), "var": (c,)}
    t = {n: torch.zeros(s) for n, s in shapes.items()}
    x, dx, skip, w, wn, z, dz, y, dy, scale, shift, mean, var = t.values()
    eng = door_engine(engine, monkeypatch, t.items())
    stats = (mean, var) if form == "bn" else ()
    for need_d, need_affine in ((True, True), (True, False), (False, False)):
        extra = {"need_affine": need_affine, **({"chunk_frames": 3} if form == "bn" else {})}
        norm = engine.BackwardNorm(scale, shift, *stats, **extra)
        if family == "unit":
            old = getattr(eng, "unit_backward_" + form)(x, w, scale, shift, *stats, dx, dskip=skip, need_du=need_d, **extra)
            new = eng.unit_backward(x, w, dx, dskip=skip, need_du=need_d, norm=norm)
        elif family == "down":
            old = getattr(eng, "down_backward_" + form)(x, w, z, scale, shift, *stats, dz, need_dx=need_d, **extra)
            new = eng.down_backward(x, w, z, dz, need_dx=need_d, norm=norm)
        else:
            old = getattr(eng, "neck_backward_" + form)(0, x, wn, scale, shift, *stats, y, dy, need_dx=need_d, **extra)
            new = eng.neck_backward(0, x, wn, y, dy, need_dx=need_d, norm=norm)
        (e0, a0), (e1, a1) = eng.log[-2:]
        assert e0 == e1 == f"pp_{family}_backward_{form}"
        assert a0 == a1
        assert [a for a in a0 if a in ("scale", "shift", "mean", "var")] == ["scale", "shift", "mean", "var"][:2 + len(stats)]
        assert [None if t is None else (t.dtype, t.shape) for t in old] == [None if t is None else (t.dtype, t.shape) for t in new]
        assert len(new) == 4 and (new[1] is None) == (not need_d) and (new[2] is None) == (not need_affine)


def test_engine_door_refuses_a_norm_with_16_bit_gradients(monkeypatch):
    engine = load_pkg("engine")
    eng = door_engine(engine, monkeypatch)
    x, w = torch.zeros(2, 64, 8, 4), torch.zeros(64, 64, 3, 3)
    norm = engine.BackwardNorm(torch.zeros(64), torch.zeros(64))
    with pytest.raises(ValueError, match="grad_precision"):
        eng.unit_backward(x, w, x, norm=norm, grad_precision="bf16")
    assert eng.log == []
