"""CPU: the plans of a training step, without an engine.  A stub engine that logs every call stands in for the device: the taps
call the RPN's autograd Function makes per frame, the engine calls of its backward with their flags, the tensors it keeps for the
backward and the parameters that end up with a gradient (the call plan); and the update_* calls that follow an optimizer step (the
upload plan).  The kernels behind these calls are timed and checked on the GPU; that a step makes exactly these calls is what keeps
its time where it is."""
import numpy as np
import pytest
import torch

from conftest import load_pkg

H, W, NB = 8, 4, 2  # the level-0 map: a canvas of 16 x 8, and level 2 is 2 x 1, still more than one element
UNITS = (3, 5, 5)
PAIRS = ((64, 64), (64, 128), (128, 256))


def level_shape(b):
    return (64 << b, H >> b, W >> b)


class StubEngine:
    """The Engine methods a training step calls, on CPU tensors: zeros of the right shapes out, every call logged with its flags."""
    grid_size = np.array([2 * H, 2 * W, 1], np.int32)
    max_batch = 8

    def __init__(self):
        self.log = []

    def effective_precision(self):
        return "fp32"

    def set_precision(self, mode):
        self.log.append(("set_precision", mode))

    def _out(self):
        return torch.zeros((1, 320, H, W)), [torch.zeros((1,) + level_shape(b)) for b in range(3)]

    def backbone(self, canvas):
        self.log.append(("backbone",))
        return self._out()[0]

    def backbone_taps(self, canvas):
        self.log.append(("backbone_taps",))
        y, xs = self._out()
        return (y, *xs)

    def backbone_block_taps(self, canvas):
        self.log.append(("backbone_block_taps",))
        y, xs = self._out()
        return (y, *xs, torch.zeros((5,) + level_shape(2)))

    def backbone_stage_taps(self, canvas):
        self.log.append(("backbone_stage_taps",))
        y, xs = self._out()
        return (y, *xs, torch.zeros((5,) + level_shape(2)), torch.zeros((1,) + level_shape(2)))

    def backbone_train_taps(self, canvas):
        self.log.append(("backbone_train_taps",))
        y, xs = self._out()
        return (y, tuple(xs), tuple(torch.zeros((n,) + level_shape(b)) for b, n in enumerate(UNITS)),
                tuple(torch.zeros((1,) + level_shape(b)) for b in range(3)))

    def neck_backward(self, branch, x, w, y, dy, need_dx=True):
        assert x.shape == (NB,) + level_shape(branch) and y.shape == dy.shape == (NB, 320, H, W)
        self.log.append(("neck_backward", branch, bool(need_dx)))
        return torch.zeros_like(w), (torch.zeros_like(x) if need_dx else None)

    def unit_backward(self, u, w, dy, dskip=None, need_du=True, grad_precision="fp32"):
        assert u.shape == dy.shape and w.shape == (u.shape[1], u.shape[1], 3, 3) and (dskip is None or dskip.shape == u.shape)
        self.log.append(("unit_backward", int(u.shape[1]), int(dskip is not None), bool(need_du), grad_precision))
        return torch.zeros_like(w), (torch.zeros_like(u) if need_du else None)

    def down_backward(self, x, w, z, dy, need_dx=True):
        assert z.shape == dy.shape and w.shape == (z.shape[1], x.shape[1], 3, 3)
        self.log.append(("down_backward", int(x.shape[1]), int(z.shape[1]), bool(need_dx)))
        return torch.zeros_like(w), (torch.zeros_like(x) if need_dx else None)

    def update_head_weights(self, sd):
        self.log.append(("update_head_weights", tuple(sd)))

    def update_neck_weights(self, params):
        self.log.append(("update_neck_weights", tuple(params)))

    def update_block_weights(self, params):
        self.log.append(("update_block_weights", tuple(params)))

    def update_down_weight(self, level, tensor):
        self.log.append(("update_down_weight", level, tuple(tensor.shape)))

    def update_rpn_weights(self, params):
        self.log.append(("update_rpn_weights", tuple(sorted(params))))

    def update_pfn_weights(self, w, gamma, beta, running_mean, running_var):
        self.log.append(("update_pfn_weights",))


def conv_shapes():
    out = []
    for b, n in enumerate(UNITS):
        cin, cout = PAIRS[b]
        out += [(cout, cin, 3, 3)] + [(cout, cout, 3, 3)] * n
    return out


def engineless(shared, loaded=False):
    """A network object assembled without an engine, its parameters in their real shapes.  loaded: as after load_state_dict, so
    that a parameter whose version moves counts as stepped."""
    net = object.__new__(shared.PointPillars)
    net.training, net._scope, net._eng = False, "head", StubEngine()
    shape = dict(zip(shared.RPN_CONV_KEYS, conv_shapes()))
    shape.update({k: (64 << b, 128 if b else 64, 1 << b, 1 << b) for b, k in enumerate(shared.NECK_KEYS)})
    shape.update({k: ((1,) if k.endswith("bias") else (1, 320, 1, 1)) for k in shared.HEAD_KEYS})
    shape.update({k: (64,) for k in shared.PFN_KEYS[1:] + shared.PFN_STAT_KEYS}, **{shared.PFN_KEYS[0]: (64, 9, 1)})
    make = lambda keys: {k: torch.nn.Parameter(torch.zeros(shape[k]), requires_grad=False) for k in keys}  # noqa: E731
    net._params, net._neck, net._block = make(shared.HEAD_KEYS), make(shared.NECK_KEYS), make(shared.BLOCK3_KEYS)
    net._down, net._rpn, net._pfn = make((shared.STAGE3_KEY,)), make(shared._RPN_EXTRA_KEYS), make(shared.PFN_KEYS)
    net._pfn_stats = {k: torch.zeros(shape[k]) for k in shared.PFN_STAT_KEYS}
    if loaded:
        net._sd = {k: np.ones(v, np.float32) for k, v in shape.items()}
        net._mark_uploaded()
    return net


def units_plan(C, dskips, last_need_du=True, prec="fp32"):
    return [("unit_backward", C, d, last_need_du or i + 1 < len(dskips), prec) for i, d in enumerate(dskips)]


def neck_plan(dx):
    return [("neck_backward", b, d) for b, d in enumerate(dx)]


def whole_plan(canvas_grad, prec="fp32"):
    return neck_plan((True, True, True)) + \
        units_plan(256, (1, 0, 1, 0, 1), prec=prec) + [("down_backward", 128, 256, True)] + \
        units_plan(128, (1, 0, 1, 0, 1), prec=prec) + [("down_backward", 64, 128, True)] + \
        units_plan(64, (1, 0, 1), prec=prec) + [("down_backward", 64, 64, canvas_grad)]


def saved_shapes(depth):
    """The shapes of what the Function keeps at a depth: y, x1..x3, the unit inputs and z of the tapped levels, the weights it was
    given, and at depth whole the canvases."""
    conv = conv_shapes()
    out = [(NB, 320, H, W)] + [(NB,) + level_shape(b) for b in range(3)] + [(64 << b, 128 if b else 64, 1 << b, 1 << b) for b in range(3)]
    if depth in ("block3", "stage3"):
        out += [(NB,) + level_shape(2)] * 5 + conv[11:]
    if depth == "stage3":
        out += [(NB,) + level_shape(2), conv[10]]
    if depth == "whole":
        out += [(NB, 64, 2 * H, 2 * W)] + conv
        for b, n in enumerate(UNITS):
            out += [(NB,) + level_shape(b)] * (n + 1)
    return sorted(out)


PLANS = {  # scope, the canvases require grad: taps call, backward calls, tensors with a .grad behind the head, depth
    ("neck", False): ("backbone_taps", neck_plan((False, False, False)), 3, "neck"),
    ("block3", False): ("backbone_block_taps", neck_plan((False, False, True)) + units_plan(256, (1, 0, 1, 0, 0), last_need_du=False), 8, "block3"),
    ("stage3", False): ("backbone_stage_taps", neck_plan((False, False, True)) + units_plan(256, (1, 0, 1, 0, 1)) +
                        [("down_backward", 128, 256, False)], 9, "stage3"),
    ("stage3", True): ("backbone_stage_taps", neck_plan((False, False, True)) + units_plan(256, (1, 0, 1, 0, 1)) +
                       [("down_backward", 128, 256, False)], 9, "stage3"),
    ("rpn", False): ("backbone_train_taps", whole_plan(False), 19, "whole"),
    ("rpn", True): ("backbone_train_taps", whole_plan(True), 19, "whole"),
    ("all", True): ("backbone_train_taps", whole_plan(True), 19, "whole"),
}


@pytest.mark.parametrize("scope,canvas_grad", list(PLANS))
def test_call_plan(scope, canvas_grad):
    shared = load_pkg("networks.pointpillars8_shared")
    taps, plan, ngrads, depth = PLANS[scope, canvas_grad]
    net = engineless(shared)
    net.train(scope=scope)
    eng = net._eng
    x = torch.zeros((NB, 64, 2 * H, 2 * W), requires_grad=canvas_grad)
    y = net.rpn_train(x)
    assert y.shape == (NB, 320, H, W) and y.requires_grad
    assert eng.log == [(taps,)] * NB  # one taps call per frame, nothing else
    assert sorted(tuple(t.shape) for t in y.grad_fn.saved_tensors) == saved_shapes(depth)
    del eng.log[:]
    y.backward(torch.ones_like(y))
    assert eng.log == plan
    behind_head = {**net._rpn, **net._down, **net._block, **net._neck}
    assert sum(p.grad is not None for p in behind_head.values()) == ngrads
    assert all((p.grad is not None) == p.requires_grad for p in behind_head.values())
    assert all(p.grad is None for p in list(net._params.values()) + list(net._pfn.values()))  # not this Function's
    assert (x.grad is not None) == (canvas_grad and depth == "whole")


def test_grad_precision_reaches_every_unit():
    shared = load_pkg("networks.pointpillars8_shared")
    net = engineless(shared)
    net.train(scope="rpn", grad_precision="bf16x3")
    y = net.rpn_train(torch.zeros((NB, 64, 2 * H, 2 * W)))
    del net._eng.log[:]
    y.backward(torch.ones_like(y))
    assert net._eng.log == whole_plan(False, prec="bf16x3")


def test_no_grad_and_eval_run_the_plain_backbone():
    shared = load_pkg("networks.pointpillars8_shared")
    net = engineless(shared)
    x = torch.zeros((NB, 64, 2 * H, 2 * W))
    assert not net.rpn_train(x).requires_grad
    net.train(scope="rpn")
    with torch.no_grad():
        assert not net.rpn_train(x).requires_grad
    net.train()  # the head alone: nothing behind it trains
    assert not net.rpn_train(x).requires_grad
    assert net._eng.log == [("backbone",)] * (3 * NB)


@pytest.mark.parametrize("scope", ["block3", "stage3", "rpn"])
def test_a_tensor_frozen_by_hand_gets_none(scope):
    """needs_input_grad per weight: a tensor frozen by hand gets no gradient, every other trained one still gets its own."""
    shared = load_pkg("networks.pointpillars8_shared")
    net = engineless(shared)
    net.train(scope=scope)
    frozen = [shared.BLOCK3_KEYS[0], shared.BLOCK3_KEYS[3], shared.NECK_KEYS[1]]
    every = {**net._rpn, **net._down, **net._block, **net._neck}
    for k in frozen:
        every[k].requires_grad_(False)
    y = net.rpn_train(torch.zeros((NB, 64, 2 * H, 2 * W)))
    y.backward(torch.ones_like(y))
    for k, p in every.items():
        assert (p.grad is not None) == p.requires_grad, k
        assert p.grad is None or p.grad.shape == p.shape, k
    assert sum(p.grad is not None for p in every.values()) == {"block3": 8, "stage3": 9, "rpn": 19}[scope] - 3


UPLOADS = {
    "head": [("update_head_weights",)],
    "neck": [("update_head_weights",), ("update_neck_weights",)],
    "block3": [("update_head_weights",), ("update_neck_weights",), ("update_block_weights",)],
    "stage3": [("update_head_weights",), ("update_neck_weights",), ("update_block_weights",), ("update_down_weight", 2)],
    "rpn": [("update_head_weights",), ("update_neck_weights",), ("update_rpn_weights",)],
    "all": [("update_head_weights",), ("update_neck_weights",), ("update_rpn_weights",)],
}


@pytest.mark.parametrize("scope", list(UPLOADS))
def test_upload_plan(scope):
    """After an optimizer step (every trainable parameter's version moved) _sync_head() and _sync_neck() make exactly the scope's
    update calls, with the tensors they carry, and a second sync makes none.  The PFN goes up with eval(), as before."""
    shared = load_pkg("networks.pointpillars8_shared")
    net = engineless(shared, loaded=True)
    eng = net._eng
    net.train(scope=scope)
    net._sync_head()
    net._sync_neck()
    assert eng.log == []  # nothing moved yet
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0)
    net._sync_head()
    net._sync_neck()
    assert [c[:2] if c[0] == "update_down_weight" else c[:1] for c in eng.log] == UPLOADS[scope]
    carried = {c[0]: c[1] for c in eng.log if c[0] != "update_down_weight"}
    assert carried["update_head_weights"] == shared.HEAD_KEYS
    assert scope == "head" or carried["update_neck_weights"] == shared.NECK_KEYS
    assert "update_block_weights" not in carried or carried["update_block_weights"] == shared.BLOCK3_KEYS
    assert "update_rpn_weights" not in carried or carried["update_rpn_weights"] == tuple(sorted(shared.RPN_CONV_KEYS))  # all sixteen
    del eng.log[:]
    net._sync_head()
    net._sync_neck()
    assert eng.log == []
    # state_dict() returns the current values (zeros; the loaded dict holds ones) for exactly the groups that were stepped
    trained = set(dict(net.named_parameters()))
    stepped = lambda: {k for k in shared.ALL_KEYS if not net.state_dict()[k].any()}  # noqa: E731
    assert stepped() == trained  # the PFN's too, which moved and has not gone up yet
    net.eval()
    assert eng.log == ([("update_pfn_weights",)] if scope == "all" else [])
    assert stepped() == trained
    # a change of precision mode commits the loaded weights again: exactly the stepped groups go up once more
    del eng.log[:]
    net.precision("fp32")
    assert eng.log == [("set_precision", "fp32")] + ([("update_pfn_weights",)] if scope == "all" else [])
    del eng.log[:]
    net._sync_head()
    net._sync_neck()
    assert [c[:2] if c[0] == "update_down_weight" else c[:1] for c in eng.log] == UPLOADS[scope]
    assert stepped() == trained
