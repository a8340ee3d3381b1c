"""CPU: the bounds and the exact data of the mixed-precision BatchNorm backwards (tests/mixedbn_ref.py) -- the restated unit bound
with no operand error against bntrain_ref / bnbatch_ref, the float64 emulation of both modes inside the bounds on every input set
tests/test_mixedbn_gpu.py uses, the representability conditions of its exact-data case -- and, without an engine, the argument rules of
train(bn_grad_precision=...), the engine door, the walk's keyword, the C ABI's declarations and a resource audit of the new kernels."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, load_pkg
import bnbatch_ref as RB
import bntrain_ref as RA
import mixedbn_ref as R
import mixedstage_ref as S
from test_bntrain_cpu import engineless
from test_head_deferred_isa_cpu import HIPCC, kernel_usage
from test_rpnwalk_cpu import door_engine

MODES = ("bf16x3", "bf16")
SYMBOLS = tuple(f"pp_{fam}_backward_{form}_mp" for fam in ("unit", "down", "neck") for form in ("affine", "bn")) + \
    tuple(f"pp_{fam}_backward_bn_path" for fam in ("unit", "down", "neck"))


def inside(got, want, bounds, what):
    for name, g, w, b in zip(("dw", "dx", "dscale", "dshift"), got, want, bounds):
        frac, dev = R.worst(g, w, b)
        print(f"{what} {name}: the emulation reaches {frac:.3f} of the bound (largest deviation {dev:.3e})")
        assert frac <= 1.0, (what, name, frac)


# ------------------------------------------------------------------ 1. the bounds
@pytest.mark.parametrize("form", R.FORMS)
def test_restated_unit_bound_is_the_references(form):
    for shape in ((64, 9, 7, 2), (128, 4, 5, 3)):
        u, w, norm, dz, dskip = R.unit_case(*shape, form)
        for skip in (None, dskip):
            want, bounds = R.unit_bounds_mixed(u, w, norm, dz, "fp32", dskip=skip)
            ref_want, ref_bounds = (RA.unit_bounds if form == "affine" else RB.unit_bounds)(u, w, *norm, dz, dskip=skip)
            for a, b in zip(want + bounds, ref_want + ref_bounds):
                assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()  # the same sums in another order of float64 additions


@functools.lru_cache(maxsize=None)
def unit_set(shape, form):
    case = R.unit_case(*shape, form)
    return case, R.unit_terms(*case[:4])


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("shape", R.UNIT_SHAPES + [R.UNIT_LARGE])
def test_unit_emulation_inside_the_bounds(shape, form):
    (u, w, norm, dz, dskip), t = unit_set(shape, form)
    for mode in MODES:
        for skip in (None, dskip) if shape != R.UNIT_LARGE else (None,):
            want, bounds = R.unit_bounds_mixed(u, w, norm, dz, mode, dskip=skip, terms=t)
            inside(R.unit_emulate(u, w, norm, dz, mode, dskip=skip), want, bounds, f"unit {form} {shape} {mode}")


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("shape", S.DOWN_SHAPES)
def test_down_emulation_inside_the_bounds(shape, form):
    x, w, z, norm, dy = R.down_case(*shape, form)
    t = R.down_terms(x, w, z, norm, dy)
    for mode in MODES:
        want, bounds = R.stage_bounds_mixed(t, mode)
        inside(R.down_emulate(x, w, z, norm, dy, mode), want, bounds, f"down {form} {shape} {mode}")


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("shape", S.NECK_MAPS)
def test_neck_emulation_inside_the_bounds(shape, form):
    xs, ws, norms, y, dy = R.neck_case(*shape, form)
    for b in range(3):
        sl = S.branch_slice(b)
        t = R.neck_terms(xs[b], ws[b], norms[b], y[:, sl], dy[:, sl])
        for mode in MODES:
            want, bounds = R.stage_bounds_mixed(t, mode)
            inside(R.neck_emulate(xs[b], ws[b], norms[b], y[:, sl], dy[:, sl], mode), want, bounds, f"neck {form} {shape} branch {b} {mode}")


def test_the_modes_can_be_told_apart():
    """bf16's operand error leaves the plain fp32 bound at UNIT_APART, and bf16x3's emulated deviation is far below bf16's."""
    u, w, norm, dz, _ = R.unit_case(*R.UNIT_APART, "affine")
    (dw, _, _, _), (bw, _, _, _) = RA.unit_bounds(u, w, *norm, dz)
    dev = {mode: np.abs(R.unit_emulate(u, w, norm, dz, mode)[0] - dw) for mode in MODES}
    assert (dev["bf16"] / bw).max() > 1.0
    assert dev["bf16x3"].max() < dev["bf16"].max() / 16


# ------------------------------------------------------------------ 2. the exact data
def survives_bf16(*ts):
    return all(np.array_equal(R.bf16_round(np.asarray(t, np.float32)), np.asarray(t, np.float32)) for t in ts)


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("shape", R.EXACT_UNITS)
def test_exact_unit_is_representable(shape, form):
    C, h, w, nb = shape
    assert (w + 2) % 8  # the row pitch is no multiple of 8: the 16-bit planes carry halo columns and the funnel shift is exercised
    u, wt, norm, dz = R.exact_unit(*shape, form)
    a = np.maximum(RA.aff(u, norm[0], norm[1]), 0.0)
    assert np.array_equal(R.a_fp32(u, norm[0], norm[1]).astype(np.float64), a)  # a is exact in float32 ...
    assert survives_bf16(a, wt, dz)  # ... and every operand has at most 8 significant bits: the bf16x3 lo parts are zero
    assert all(np.array_equal(R.bf16_split(np.asarray(t, np.float32))[1], np.zeros_like(t, np.float32)) for t in (a, wt, dz))
    assert (a > 0).mean() > 0.2 and (a == 0).mean() > 0.2  # both branches of the ReLU
    assert R.exact_margin(dz, a, nb * h * w) < 1 and R.exact_margin(dz, wt, 9 * C) < 1  # every partial sum is exact in float32
    g = R.B.conv3_dgrad(np.asarray(dz, np.float64), np.asarray(wt, np.float64)) * (a > 0)
    assert np.array_equal((RA.ch(norm[0]) * g).astype(np.float32).astype(np.float64), RA.ch(norm[0]) * g)  # scale g too


@pytest.mark.parametrize("shape", R.EXACT_DOWNS)
def test_exact_down_is_representable(shape):
    cin, cout, hin, win, nb = shape
    x, wt, z, norm, dy = R.exact_down(*shape)
    dz = RA.ch(norm[0]) * (dy * (RA.aff(z, norm[0], norm[1]) > 0))
    assert survives_bf16(x, wt, dz)
    assert R.exact_margin(dz, x, nb * ((hin + 1) // 2) * ((win + 1) // 2)) < 1 and R.exact_margin(dz, wt, 4 * cout) < 1


def test_exact_neck_is_representable():
    H, W, nb = R.EXACT_NECK
    xs, ws, norms, y, dy = R.exact_neck(H, W, nb)
    for b in range(3):
        sl = S.branch_slice(b)
        dz = RA.ch(norms[b][0]) * (dy[:, sl] * (y[:, sl] > 0))
        assert survives_bf16(xs[b], ws[b], dz) and 0.2 < (y[:, sl] > 0).mean() < 0.8
        assert R.exact_margin(xs[b], ws[b], xs[b].shape[1]) < 1  # Z, recomputed in float32, is exact
        assert R.exact_margin(dz, xs[b], nb * (H >> b) * (W >> b)) < 1 and R.exact_margin(dz, ws[b], ws[b].shape[1] << (2 * b)) < 1


# ------------------------------------------------------------------ 3. train(), the engine door and the walk
def test_train_argument_rules():
    shared = load_pkg("networks.pointpillars8_shared")
    bn = engineless(load_pkg("networks.pointpillars8_export").PointPillars, shared)
    trt = engineless(load_pkg("networks.pointpillars8_trt").PointPillars, shared)
    inn = engineless(shared.PointPillars, shared)
    for net in (bn, trt):
        assert net.bn_grad_precision == "fp32"
        for stats in ("frozen", "moving"):
            for prec in shared.GRAD_PRECISIONS:
                for stages in shared.GRAD_STAGES:
                    assert net.train(scope="rpn", bn_stats=stats, bn_grad_precision=prec, grad_stages=stages) is net
                    assert (net.bn_grad_precision, net.grad_stages, net.grad_precision, net.bn_stats) == (prec, stages, "fp32", stats)
            assert net.train(scope="rpn", bn_stats=stats).bn_grad_precision == "fp32"  # the default
            with pytest.raises(ValueError, match="bn_grad_precision"):
                net.train(scope="rpn", bn_stats=stats, bn_grad_precision="fp16")
            with pytest.raises(ValueError, match="fp32"):  # grad_precision stays refused on these networks
                net.train(scope="rpn", bn_stats=stats, grad_precision="bf16", bn_grad_precision="bf16")
        with pytest.raises(ValueError, match="bn_stats"):
            net.train(scope="head", bn_grad_precision="bf16")
        net.train(scope="rpn", bn_stats="moving", bn_grad_precision="bf16", grad_stages="rpn")
        net.eval()
        assert (net.bn_grad_precision, net.grad_stages, net.bn_stats, net.training) == ("fp32", "units", None, False)
    for prec in MODES:
        with pytest.raises(ValueError, match="grad_precision"):
            inn.train(scope="rpn", bn_grad_precision=prec)
    assert inn.train(scope="rpn", grad_precision="bf16", bn_grad_precision="fp32").grad_precision == "bf16"
    with pytest.raises(ValueError, match="bn_grad_precision"):
        inn.train(scope="rpn", bn_grad_precision="fp64")


def test_engine_door(monkeypatch):
    """norm= with bn_grad_precision reaches the _mp entry with the mode in front; "fp32" reaches the fp32 entry as before."""
    engine = load_pkg("engine")
    eng = door_engine(engine, monkeypatch)
    c = 64
    x, w, wn, z, y = torch.zeros(2, c, 8, 4), torch.zeros(c, c, 3, 3), torch.zeros(c, c, 1, 1), torch.zeros(2, c, 4, 2), torch.zeros(2, 320, 8, 4)
    v = torch.zeros(c)
    for form, norm in (("affine", engine.BackwardNorm(v, v)), ("bn", engine.BackwardNorm(v, v, v, v))):
        for prec, mode in engine.Engine.GRAD_PRECISIONS.items():
            eng.log.clear()
            assert len(eng.unit_backward(x, w, x, norm=norm, bn_grad_precision=prec)) == 4
            assert len(eng.down_backward(x, w, z, z, norm=norm, bn_grad_precision=prec)) == 4
            assert len(eng.neck_backward(0, x, wn, y, y, norm=norm, bn_grad_precision=prec)) == 4
            mp = "_mp" if mode else ""
            assert [e for e, _ in eng.log] == [f"pp_{fam}_backward_{form}{mp}" for fam in ("unit", "down", "neck")]
            assert [a[0] for _, a in eng.log] == ([mode] * 3 if mode else [c, c, 0])  # the mode leads; without one the first int of the shape
        eng.log.clear()
        with pytest.raises(ValueError, match="bn_grad_precision"):
            eng.unit_backward(x, w, x, norm=norm, bn_grad_precision="fp16")
    with pytest.raises(ValueError, match="norm"):
        eng.unit_backward(x, w, x, bn_grad_precision="bf16")  # without a norm the keyword is grad_precision
    assert eng.log == []


def test_walk_hands_the_keyword_to_layers_with_a_norm():
    """_layer_backward: a layer with a norm gets bn_grad_precision only when a precision is given, one without gets grad_precision."""
    shared = load_pkg("networks.pointpillars8_shared")
    engine = load_pkg("engine")
    seen = []

    def primitive(*args, **kw):
        seen.append(kw)
        return (0, 1, 2, 3) if "norm" in kw else (0, 1)

    norm = engine.BackwardNorm(None, None, need_affine=False)
    shared._layer_backward(None, primitive, shared._Layer(None, True, norm), 5)
    shared._layer_backward(None, primitive, shared._Layer(None, True, norm), 5, prec="bf16")
    shared._layer_backward(None, primitive, shared._Layer(None, True), 5, prec="bf16")
    assert seen == [{"norm": norm}, {"norm": norm, "bn_grad_precision": "bf16"}, {"grad_precision": "bf16"}]


# ------------------------------------------------------------------ 4. ABI and resources
def test_c_abi_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    protos = load_pkg("_lib").PROTOTYPES
    for name in SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name + " is not declared in include/pp_hip.h"
        args = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]
        assert name in protos and len(protos[name][1]) == len(args), (name, len(args))
        assert args[1].split() == ["int", "mode"], name  # directly behind the context
        if name.endswith("_mp"):  # the fp32 sibling's list with the mode put in
            sib = protos[name[:-3]][1]
            assert protos[name][1] == sib[:1] + [protos[name][1][1]] + sib[1:], name
    so = os.path.join(ROOT, "3d_object_detection_amd", "csrc", "libpp_hip.so")
    if not os.path.exists(so):
        pytest.skip("libpp_hip.so is not built")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert re.search(r"\bT " + name + r"$", exported, re.M), name + " is not exported"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_new_streaming_kernels_use_no_scratch():
    k = {n: u for n, u in kernel_usage("block_train16.hip").items() if "k_affine_unit_pack16" in n or "k_affine_unit_du" in n}
    print(k)
    assert sum("k_affine_unit_pack16" in n for n in k) == 2 and sum("k_affine_unit_du" in n for n in k) == 1, sorted(k)
    for n, u in k.items():
        assert u["ScratchSize [bytes/lane]"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (n, u)
