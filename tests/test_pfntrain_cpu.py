"""CPU: the float64 restatement of the pillar feature net in train mode and of its closed-form backward (tests/pfntrain_ref.py) against
the reference's float64 autograd goldens (tests/golden/pfntrain_small.npz, tests/golden/make_pfntrain_goldens.py); the fixture's seed
and margins; the key order and the parameter bookkeeping of train(scope="all") on a network object assembled without an engine; the C
ABI's declarations; and a resource audit of the kernels of csrc/pfn_train.hip."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, golden, load_pkg
import pfntrain_ref as R
from test_head_deferred_isa_cpu import HIPCC, kernel_usage
from test_rpntrain_cpu import engineless

sys.path.insert(0, GOLDEN)
from make_pfntrain_goldens import CASES, MARGIN, NAMES, SEED, geometry, small_inputs  # noqa: E402

SYMBOLS = ("pp_pfn_train_forward", "pp_scatter_backward", "pp_pfn_backward", "pp_update_pfn_weights")


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def restate(case, seed=None):
    inp = small_inputs(case, seed)
    f = R.features(inp["voxels"], inp["coors"], inp["npts"], *geometry())
    fwd = R.forward(f, inp["w"], inp["gamma"], inp["beta"])
    dw, dg, db = R.backward(f, inp["w"], inp["gamma"], fwd, inp["g"])
    return inp, f, fwd, dict(dw=dw, dgamma=dg, dbeta=db, feat=fwd["feat"], mean=fwd["mean"], var=fwd["var"])


@pytest.mark.parametrize("case", list(CASES))
def test_restatement_matches_the_reference(case):
    g = golden("pfntrain_small")
    inp, f, fwd, got = restate(case)
    spec = CASES[case]
    assert inp["voxels"].shape == (sum(spec["frames"]), spec["T"], 4) and set(spec["forced"](spec["T"])) <= set(inp["npts"].tolist())
    assert len({(f, x, y) for f, (x, y, _) in zip(inp["frame"], inp["coors"])}) == len(inp["coors"])  # distinct cells per frame
    for k in NAMES:
        assert got[k].shape == g[f"{k}_{case}"].shape and rel(got[k], g[f"{k}_{case}"]) <= 1e-10, k
        assert 0 < float(g[f"ref32_dev_{k}_{case}"]) < 1e-5, k
    assert np.array_equal(fwd["arg"], g["arg_" + case])
    init = load_pkg("networks.init").init_state_dict(0, norm="instance")
    rm, rv = R.running(init["pillar_point_net.pfn_layers.1.running_mean"], init["pillar_point_net.pfn_layers.1.running_var"], fwd)
    assert rel(rm, g["rm_" + case]) <= 1e-10 and rel(rv, g["rv_" + case]) <= 1e-10
    # a backward evaluated at the forward's own selection, handed in, is the same backward
    again = R.backward(f, inp["w"], inp["gamma"], fwd, inp["g"], arg=fwd["arg"])
    assert all(np.array_equal(a, got[k]) for a, k in zip(again, ("dw", "dgamma", "dbeta")))
    # what the fixture must exercise: a padded slot that wins, and a channel the ReLU switches off
    n = inp["npts"].astype(np.int64)[:, None]
    assert ((fwd["arg"] == n) & (n < spec["T"]) & (fwd["feat"] > 0)).any() and (fwd["feat"] == 0).any()
    # the padded slots are what BatchNorm1d sees as zeros: z = 0 there
    pad = np.arange(spec["T"])[None, :] >= n
    assert np.all(fwd["z"][pad] == 0.0)


def test_seed_and_margins():
    g = golden("pfntrain_small")
    assert int(g["seed"]) == SEED
    for case in CASES:
        inp, _, fwd, _ = restate(case)
        gap, top = R.margins(fwd["y"], inp["npts"])
        assert gap >= MARGIN and top >= MARGIN, (case, gap, top)
        assert abs(gap - float(g["gap_" + case])) <= 1e-9 and abs(top - float(g["top_" + case])) <= 1e-9
    for seed in range(11, SEED):  # the first from 11 upward: every earlier one misses a margin in one of the cases
        miss = []
        for case in CASES:
            inp, _, fwd, _ = restate(case, seed)
            miss.append(min(R.margins(fwd["y"], inp["npts"])) < MARGIN)
        assert any(miss), seed


def test_key_order_is_the_reference_state_dict_order():
    shared = load_pkg("networks.pointpillars8_shared")
    eng = load_pkg("engine").Engine
    keys = [str(k) for k in golden("pfntrain_small")["state_dict_keys"]]
    assert len(keys) == 28 and list(shared.ALL_KEYS) == keys
    assert list(shared.PFN_KEYS) == keys[:3] and shared.PFN_KEYS is eng.PFN_KEYS and list(shared.RPN_KEYS) == keys[3:]
    sd = load_pkg("networks.init").init_state_dict(0, norm="instance")
    assert all(k in sd for k in keys) and all(k in sd for k in shared.PFN_STAT_KEYS)
    assert sd[keys[0]].shape == (64, 9, 1) and sd[keys[1]].shape == (64,) and sd[keys[2]].shape == (64,)


def test_all_scope_parameters():
    """Parameter counts and requires_grad under train(scope="all"), on a network object assembled without an engine."""
    shared = load_pkg("networks.pointpillars8_shared")
    net = engineless(shared)
    with pytest.raises(RuntimeError):
        net.train(scope="all")  # no pillar feature net in this object yet
    net._pfn = {k: torch.nn.Parameter(torch.zeros(1), requires_grad=False) for k in shared.PFN_KEYS}
    net._pfn_stats = {k: torch.zeros(1) for k in shared.PFN_STAT_KEYS}
    net.train(scope="all")
    assert [k for k, _ in net.named_parameters()] == list(shared.ALL_KEYS)
    assert len(list(net.parameters())) == 28 and all(p.requires_grad for p in net.parameters())
    net.train(scope="rpn")
    assert [k for k, _ in net.named_parameters()] == list(shared.RPN_KEYS) and not any(p.requires_grad for p in net._pfn.values())
    net.eval()
    assert not any(p.requires_grad for p in net._pfn.values())
    with pytest.raises(ValueError, match="'all'"):
        net.train(scope="bogus")


def test_c_abi_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    lib_mod = load_pkg("_lib")
    lib = lib_mod.load()
    for name in SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name + " is not declared in include/pp_hip.h"
        nargs = len([a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()])
        assert name in lib_mod.PROTOTYPES and len(lib_mod.PROTOTYPES[name][1]) == nargs, (name, nargs)
        assert hasattr(lib, name), name
    assert int(re.search(r"#define PP_PFN_STATS (\d+)", hdr).group(1)) == load_pkg("engine").Engine.PFN_STATS == 64 + 64 + 9 + 81


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_pfn_train_kernels_use_no_scratch():
    """The statistics pass keeps 54 fp64 accumulators per lane, the backward 11: they must stay in registers."""
    k = kernel_usage("pfn_train.hip")
    names = ("pfn_stats_kernel", "pfn_stats_finish", "pfn_train_kernel", "scatter_bwd_kernel", "pfn_bwd_kernel", "pfn_bwd_finish", "pfn_fold_kernel")
    print(k)
    for want in names:
        hit = [u for n, u in k.items() if want in n]
        assert len(hit) == 1, (want, sorted(k))
        assert hit[0]["ScratchSize [bytes/lane]"] == "0" and hit[0]["VGPRs Spill"] == "0" and hit[0]["SGPRs Spill"] == "0", (want, hit[0])
