"""CPU: train(forward_precision=...) as a plan of engine calls, with the stub engine of tests/test_trainplan_cpu.py.  Under the default
a training step makes today's calls, name for name and argument for argument: the stub has today's signatures, so a keyword that
reached it would raise.  Under a 16-bit forward_precision the sequence is the same with the mode on the taps and upload calls only;
the keyword is "fp32" again after eval(); and what is no mode is refused before any engine call."""
import os

import pytest
import torch

from conftest import ROOT, load_pkg
import test_trainplan_cpu as P

MODES = ("bf16x3", "bf16", "fp16")


class ModeEngine(P.StubEngine):
    """P.StubEngine with a precision mode and the forward_precision keyword: a call that carries a mode logs it as its last entry."""

    def __init__(self):
        super().__init__()
        self.mode = "fp32"

    def effective_precision(self):
        return self.mode

    def set_precision(self, mode):
        super().set_precision(mode)
        self.mode = mode

    def _with_mode(self, name, args, forward_precision):
        n = len(self.log)
        out = getattr(P.StubEngine, name)(self, *args)
        if forward_precision != "fp32":
            assert forward_precision == self.mode, "the engine would refuse another mode than the plan's"
            self.log[n] = self.log[n] + (forward_precision,)
        return out

    def backbone_train_taps(self, canvas, forward_precision="fp32"):
        return self._with_mode("backbone_train_taps", (canvas,), forward_precision)

    def update_head_weights(self, sd, forward_precision="fp32"):
        return self._with_mode("update_head_weights", (sd,), forward_precision)

    def update_neck_weights(self, params, forward_precision="fp32"):
        return self._with_mode("update_neck_weights", (params,), forward_precision)

    def update_rpn_weights(self, params, forward_precision="fp32"):
        return self._with_mode("update_rpn_weights", (params,), forward_precision)


def one_step(net, **train_kw):
    """train(), a forward and backward of the RPN, an optimizer step, the uploads -> the engine's log."""
    net.train(**train_kw)
    y = net.rpn_train(torch.zeros((P.NB, 64, 2 * P.H, 2 * P.W)))
    y.backward(torch.ones_like(y))
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0)
    net._sync_head()
    net._sync_neck()
    return list(net._eng.log)


def todays_step(scope):
    taps, plan, _, _ = P.PLANS[scope, False]
    return [(taps,)] * P.NB + plan


@pytest.mark.parametrize("scope", ["neck", "block3", "stage3", "rpn"])
def test_the_default_makes_todays_calls(scope):
    shared = load_pkg("networks.pointpillars8_shared")
    net = P.engineless(shared, loaded=True)  # today's stub: no method takes forward_precision
    log = one_step(net, scope=scope)
    n = P.NB + len(P.PLANS[scope, False][1])
    assert log[:n] == todays_step(scope)
    assert [c[:2] if c[0] == "update_down_weight" else c[:1] for c in log[n:]] == P.UPLOADS[scope]
    assert net.forward_precision == "fp32"
    other = P.engineless(shared, loaded=True)
    other._eng = ModeEngine()
    assert one_step(other, scope=scope, forward_precision="fp32") == log  # the keyword spelled out changes nothing


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("grad", ["fp32", "bf16", "bf16x3"])
def test_a_16_bit_forward_adds_the_mode_to_taps_and_uploads_only(mode, grad):
    shared = load_pkg("networks.pointpillars8_shared")
    base = P.engineless(shared, loaded=True)
    base._eng = ModeEngine()
    kw = {"scope": "rpn", "grad_precision": grad}  # combines freely with the precision of the unit backwards
    want = one_step(base, **kw)
    net = P.engineless(shared, loaded=True)
    net._eng = ModeEngine()
    got = one_step(net, **kw, forward_precision=mode)
    assert got[0] == ("set_precision", mode) and net._eng.mode == mode and net.forward_precision == mode
    got = got[1:]
    assert len(got) == len(want)
    carries = {"backbone_train_taps", "update_head_weights", "update_neck_weights", "update_rpn_weights"}
    for g, w in zip(got, want):
        assert g == (w + (mode,) if w[0] in carries else w), (g, w)
    assert sum(g[0] in carries for g in got) == P.NB + 3
    # already in the mode: no second switch
    del net._eng.log[:]
    net.train(scope="rpn", forward_precision=mode)
    assert net._eng.log == []


@pytest.mark.parametrize("scope,uploads", [("neck", 2), ("block3", 3), ("stage3", 3)])
def test_narrower_scopes_tap_every_level_and_upload_by_family(scope, uploads):
    """A 16-bit forward has the one tapped pass (pp_backbone_train_taps_mp); the backward is the scope's own plan; block 3's and the
    stage's weights go up with all sixteen convolutions (pp_update_rpn_weights_mp), once."""
    shared = load_pkg("networks.pointpillars8_shared")
    net = P.engineless(shared, loaded=True)
    net._eng = ModeEngine()
    log = one_step(net, scope=scope, forward_precision="fp16")
    plan = P.PLANS[scope, False][1]
    assert log[0] == ("set_precision", "fp16")
    assert log[1:1 + P.NB] == [("backbone_train_taps", "fp16")] * P.NB
    assert log[1 + P.NB:1 + P.NB + len(plan)] == plan
    ups = log[1 + P.NB + len(plan):]
    assert [c[0] for c in ups] == ["update_head_weights", "update_neck_weights", "update_rpn_weights"][:uploads]
    assert all(c[-1] == "fp16" for c in ups)


def test_the_keyword_resets_after_eval_and_uploads_follow_the_engine():
    shared = load_pkg("networks.pointpillars8_shared")
    net = P.engineless(shared, loaded=True)
    eng = net._eng = ModeEngine()
    net.train(scope="rpn", forward_precision="bf16")
    assert (net.forward_precision, eng.mode) == ("bf16", "bf16")
    net.eval()
    assert net.forward_precision == "fp32" and eng.mode == "bf16"  # eval() leaves the engine where it is
    assert net.train(scope="rpn").forward_precision == "fp32"
    with pytest.raises(RuntimeError, match="fp32"):  # today's wording: the engine runs bf16, the keyword says fp32
        net.rpn_train(torch.zeros((P.NB, 64, 2 * P.H, 2 * P.W)))
    net.precision("fp32")
    # stepped in fp32, then switched: the uploads pick the entry by the engine's mode, in eval mode too
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0)
    net.eval()
    net.precision("fp16")
    del eng.log[:]
    net._sync_head()
    net._sync_neck()
    assert [c[0] for c in eng.log] == ["update_head_weights", "update_neck_weights", "update_rpn_weights"] and all(c[-1] == "fp16" for c in eng.log)
    net.precision("fp16s")
    with pytest.raises(RuntimeError, match="load_state_dict"):
        net._sync_head()
    # a 16-bit training forward whose engine was switched away
    net.precision("fp32")
    net.train(scope="rpn", forward_precision="fp16")
    net.precision("fp32")
    with pytest.raises(RuntimeError, match="fp16"):
        net.rpn_train(torch.zeros((P.NB, 64, 2 * P.H, 2 * P.W)))


def test_argument_validation():
    shared = load_pkg("networks.pointpillars8_shared")
    net = P.engineless(shared)
    for bad in ("fp16s", "half", None, 3):
        with pytest.raises(ValueError, match="forward_precision"):
            net.train(scope="rpn", forward_precision=bad)
    assert net._eng.log == [] and not net.training

    class Batch(shared.PointPillars):
        _norm = "batch"

    bn = object.__new__(Batch)
    bn.training, bn._scope, bn._eng = False, "head", P.StubEngine()
    for kw in ({}, {"scope": "rpn", "bn_stats": "frozen"}):
        with pytest.raises(ValueError, match="forward_precision"):
            bn.train(forward_precision="fp16", **kw)
    assert bn._eng.log == []
    # the engine's own door
    engine = load_pkg("engine")
    eng = object.__new__(engine.Engine)
    eng.effective_precision = lambda: "bf16"
    assert eng._forward_mode("fp32", "x") == 0 and eng._forward_mode("bf16", "x") == 2
    for bad in ("fp16s", "half", None):
        with pytest.raises(ValueError, match="forward_precision"):
            eng._forward_mode(bad, "x")
    with pytest.raises(RuntimeError, match="'fp16'.*'bf16'"):
        eng._forward_mode("fp16", "x")


def test_the_entries_are_declared_and_built():
    protos = load_pkg("_lib").PROTOTYPES
    header = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    lib = os.path.join(ROOT, "3d_object_detection_amd", "csrc", "libpp_hip.so")
    built = open(lib, "rb").read() if os.path.exists(lib) else None
    for name in ("pp_backbone_train_taps_mp", "pp_update_rpn_weights_mp", "pp_update_neck_weights_mp", "pp_update_head_weights_mp", "pp_debug_image16"):
        assert name in protos and f"int {name}(" in header, name
        assert built is None or name.encode() in built, name
