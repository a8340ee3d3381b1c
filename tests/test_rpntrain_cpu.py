"""CPU: the float64 restatement of the whole RPN backward (tests/rpntrain_ref.py, composed from necktrain_ref, blocktrain_ref and
downtrain_ref by the table the network's _RpnFunction walks) against the reference's float64 autograd goldens
(tests/golden/rpntrain_small.npz, tests/golden/make_rpntrain_goldens.py): the wiring -- residual adds, unit order, where an
upsampler's dx joins.  Also the key order and the parameter bookkeeping of train(scope="rpn") on a network object assembled without an
engine, the C ABI's declarations, and a resource audit of the new and changed kernels: the image kernel of csrc/sparse_conv1.hip and
the segmented streaming passes of csrc/block_train.hip and csrc/down_train.hip."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, golden, load_pkg
import rpntrain_ref as R
from test_head_deferred_isa_cpu import HIPCC, kernel_usage

sys.path.insert(0, GOLDEN)
from make_rpntrain_goldens import DW_STRIDE, DX_STRIDE, SEED, small_inputs, split, weight_shapes  # noqa: E402

SYMBOLS = ("pp_backbone_train_taps", "pp_update_rpn_weights")


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.fixture(scope="module")
def restated():
    canvas, ws, dy = small_inputs()
    wc, wn = split(ws)
    fwd = R.rpn_forward(canvas, wc, wn)
    dwc, dwn, dx = R.rpn_backward(canvas, wc, wn, fwd, dy)
    return dict(fwd=fwd, dw={**dict(zip(R.CONV_KEYS, dwc)), **dict(zip(R.NECK_KEYS, dwn))}, dx=dx, ws=ws)


def test_restatement_matches_the_reference(restated):
    g = golden("rpntrain_small")
    assert int(g["seed"]) == SEED and int(g["dw_stride"]) == DW_STRIDE and int(g["dx_stride"]) == DX_STRIDE
    assert [tuple(w.shape) for w in restated["ws"]] == weight_shapes()
    for i, k in enumerate(R.KEYS):
        dw = restated["dw"][k]
        assert dw.shape == restated["ws"][i].shape, k
        assert rel(dw.reshape(-1)[::DW_STRIDE], g[f"dw_{i}"]) <= 1e-10, k
        assert abs(np.abs(dw).max() - float(g[f"dw_{i}_max"])) <= 1e-10 * np.abs(dw).max(), k
    dx = restated["dx"]
    assert rel(dx.reshape(-1)[::DX_STRIDE], g["dcanvas"]) <= 1e-10
    assert abs(np.abs(dx).max() - float(g["dcanvas_max"])) <= 1e-10 * np.abs(dx).max()


def test_forward_tensors_and_masks(restated):
    """The tensors the restated forward hands out have the shapes of the taps, units_b[0] is the stage's output, and every ReLU site
    is listed once."""
    fwd = restated["fwd"]
    assert [len(u) for u in fwd["units"]] == [3, 5, 5] and fwd["y"].shape == (2, 320, 16, 12)
    for b in range(3):
        shape = (2, 64 << b, 16 >> b, 12 >> b)
        assert fwd["zs"][b].shape == shape and fwd["taps"][b].shape == shape and all(u.shape == shape for u in fwd["units"][b])
        assert np.array_equal(fwd["units"][b][0], np.maximum(R.B.norm(fwd["zs"][b])[0], 0.0))
    masks = R.relu_masks(fwd["y"], fwd["units"], fwd["zs"])
    assert len(masks) == 19 and all(0 < m.mean() < 1 for m in masks.values())


def test_key_order_is_the_reference_state_dict_order():
    shared = load_pkg("networks.pointpillars8_shared")
    eng = load_pkg("engine").Engine
    keys = [str(k) for k in golden("rpntrain_small")["state_dict_keys"]]
    assert len(keys) == 25 and list(shared.RPN_KEYS) == keys
    assert len(eng.RPN_CONV_KEYS) == 16 and list(eng.RPN_CONV_KEYS) == [k for k in keys if k.startswith("rpn.block")]
    assert shared.RPN_CONV_KEYS is eng.RPN_CONV_KEYS and list(R.CONV_KEYS) == list(eng.RPN_CONV_KEYS)
    assert list(R.KEYS) == keys[:19] and R.RPN_TABLE == shared.RPN_TABLE
    assert eng.RPN_UNITS == tuple(sum(mods) for _, mods in shared.RPN_TABLE)
    sd = load_pkg("networks.init").init_state_dict(0, norm="instance")
    assert sorted(k for k in sd if k in shared.RPN_KEYS) == sorted(keys)  # every one is a tensor of this project's state_dict


def engineless(shared):
    net = object.__new__(shared.PointPillars)
    net.training, net._scope = False, "head"
    zeros = lambda keys: {k: torch.nn.Parameter(torch.zeros(1), requires_grad=False) for k in keys}  # noqa: E731
    net._params, net._neck, net._block = zeros(shared.HEAD_KEYS), zeros(shared.NECK_KEYS), zeros(shared.BLOCK3_KEYS)
    net._down, net._rpn = zeros((shared.STAGE3_KEY,)), zeros(shared._RPN_EXTRA_KEYS)
    return net


def test_rpn_scope_parameters():
    """Parameter counts and requires_grad per scope, on a network object assembled without an engine: no GPU here."""
    shared = load_pkg("networks.pointpillars8_shared")
    net = engineless(shared)
    every = lambda: list(net._rpn.values()) + list(net._down.values()) + list(net._block.values()) + list(net._neck.values())  # noqa: E731
    assert len(net._rpn) == 10
    for scope, count in (("head", 6), ("neck", 9), ("block3", 14), ("stage3", 15), ("rpn", 25)):
        net.train(scope=scope)
        params = list(net.parameters())
        assert len(params) == count and all(p.requires_grad for p in params), scope
        assert sum(p.requires_grad for p in every()) == count - 6, scope
    net.train(scope="rpn")
    assert [k for k, _ in net.named_parameters()] == list(shared.RPN_KEYS)
    net.eval()
    assert [k for k, _ in net.named_parameters()] == list(shared.HEAD_KEYS)
    assert not any(p.requires_grad for p in every() + list(net._params.values()))
    with pytest.raises(ValueError):
        net.train(scope="backbone")
    with pytest.raises(ValueError):
        net.train(scope="block1")
    # a network without the ten tensors of blocks 1 and 2 (the BatchNorm export folds them) cannot train the rpn
    net._rpn = {}
    with pytest.raises(RuntimeError, match="InstanceNorm"):
        net.train(scope="rpn")
    net.train(scope="stage3")


def test_c_abi_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    protos = load_pkg("_lib").PROTOTYPES
    for name in SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name + " is not declared in include/pp_hip.h"
        nargs = len([a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()])
        assert name in protos and len(protos[name][1]) == nargs, (name, nargs)
    # the refusals of the narrower entry points are part of their contract
    blk = open(os.path.join(ROOT, "3d_object_detection_amd", "csrc", "block_train.hip")).read()
    dwn = open(os.path.join(ROOT, "3d_object_detection_amd", "csrc", "down_train.hip")).read()
    assert "pp_update_block_weights: block 3 only" in blk and "pp_update_down_weight: level 2 only" in dwn


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_first_conv_image_kernel_uses_no_scratch():
    k = {n: u for n, u in kernel_usage("sparse_conv1.hip").items() if "first_conv_image" in n}
    print(k)
    assert len(k) == 2, sorted(k)  # kc = 4 and 8
    for n, u in k.items():
        assert u["ScratchSize [bytes/lane]"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (n, u)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src,names", [("block_train.hip", ("k_plane_stats", "k_plane_gstats", "k_unit_pack", "k_unit_norm")),
                                       ("down_train.hip", ("k_plane_stats", "k_dplane_gstats", "k_down_xpack", "k_down_norm"))])
def test_segmented_passes_use_no_scratch(src, names):
    k = {n: u for n, u in kernel_usage(src).items() if any(m in n for m in names)}
    print(k)
    assert len(k) == 4, sorted(k)
    for n, u in k.items():
        assert u["ScratchSize [bytes/lane]"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (n, u)
