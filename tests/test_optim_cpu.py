"""CPU (-m "not gpu"): the float64 restatement of the device optimizer (tests/optim_ref.py) against torch's own float64 run of
clip_grad_norm_ + Adam / AdamW; the state_dict layout of framework.optim against torch.optim in both directions, on CPU tensors; and
the refusals that need no GPU."""
import copy

import numpy as np
import pytest
import torch

from conftest import load_pkg
import optim_ref as R

OPT = load_pkg("framework.optim")
CHUNK = load_pkg("_lib").PP_OPT_CHUNK
VARIANTS = {"adam": ("Adam", 0.0), "adam_l2": ("Adam", 1e-2), "adamw": ("AdamW", 1e-2)}


def torch_params(entries, dtype, with_grad=True):
    ps = [torch.nn.Parameter(torch.from_numpy(np.array(e["p"])).to(dtype)) for e in entries]
    if with_grad:
        for q, e in zip(ps, entries):
            q.grad = None if e["g"] is None else torch.from_numpy(np.array(e["g"])).to(dtype)
    return ps


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_restatement_equals_torch_float64(variant):
    name, wd = VARIANTS[variant]
    entries = R.main_list(CHUNK)
    ps = torch_params(entries, torch.float64)
    opt = getattr(torch.optim, name)(ps, lr=1e-3, weight_decay=wd)
    mine = [dict(p=np.array(e["p"], np.float64), m=np.zeros(e["p"].shape), v=np.zeros(e["p"].shape)) for e in entries]
    norm0 = R.total_norm([e["g"] for e in entries])
    worst = 0.0
    for k, max_norm in enumerate((0.5 * norm0, 10.0, 1.2 * norm0)):  # clipped, not clipped, clipped again (the gradients grow)
        scale = 1.0 + 0.5 * k
        for q, e in zip(ps, entries):
            q.grad = None if e["g"] is None else torch.from_numpy(np.array(e["g"], np.float64) * scale)
        want_norm = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
        opt.step()
        grads = [None if e["g"] is None else np.array(e["g"], np.float64) * scale for e in entries]
        norm = R.total_norm(grads)
        assert abs(norm - want_norm) <= 1e-12 * want_norm
        coef = R.clip_coef(norm, max_norm)
        assert (coef < 1.0) == (k != 1)
        for q, s, g in zip(ps, mine, grads):
            if g is None:
                assert len(opt.state[q]) == 0
                continue
            s["p"], s["m"], s["v"] = R.adam_step(s["p"], g, s["m"], s["v"], k + 1, lr=1e-3, weight_decay=wd, decoupled=name == "AdamW", coef=coef)
            if s["p"].size == 0:
                continue
            st = opt.state[q]
            assert int(st["step"]) == k + 1
            for got, want in ((s["p"], q.detach()), (s["m"], st["exp_avg"]), (s["v"], st["exp_avg_sq"])):
                want = want.numpy()
                top = float(np.abs(want).max())  # zero for the moments of the one-element tensor, whose gradient is exactly 0
                worst = max(worst, float(np.abs(got - want).max()) / (top if top > 0 else 1.0))
    print(f"{variant}: restatement against torch float64, worst deviation {worst:.2e} of a tensor's maximum")
    assert worst <= 1e-12


def test_clip_coef():
    assert R.clip_coef(0.0, 10.0) == 1.0 and R.clip_coef(20.0, 10.0) == 10.0 / (20.0 + 1e-6)
    assert np.isnan(R.clip_coef(float("nan"), 10.0)) and R.clip_coef(float("inf"), 10.0) == 0.0


def same_state(a, b):
    """Two optimizer state dicts: equal keys, tensors, step counts and param_groups."""
    assert list(a["state"]) == list(b["state"])
    for i in a["state"]:
        assert set(a["state"][i]) == set(b["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        for k in a["state"][i]:
            x, y = a["state"][i][k], b["state"][i][k]
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (i, k)
    assert len(a["param_groups"]) == len(b["param_groups"]) == 1
    ga, gb = a["param_groups"][0], b["param_groups"][0]
    assert list(ga) == list(gb), (list(ga), list(gb))
    assert all(ga[k] == gb[k] for k in ga), (ga, gb)


@pytest.mark.parametrize("name", ["Adam", "AdamW"])
def test_state_interop(name):
    entries = [e for e in R.main_list(CHUNK) if e["kind"] != "view"][:8] + [R.main_list(CHUNK)[-1]]  # the last one has no gradient
    ps = torch_params(entries, torch.float32)
    theirs = getattr(torch.optim, name)(ps, lr=2e-3)
    for _ in range(2):
        theirs.step()
    sd = copy.deepcopy(theirs.state_dict())  # state_dict() hands out the live tensors, and load_state_dict keeps them where it can
    assert len(sd["state"]) == len(entries) - 1 and float(sd["state"][0]["step"]) == 2.0
    ours = getattr(OPT, name)(torch_params(entries, torch.float32, with_grad=False), lr=7e-3)
    assert list(ours.state_dict()["param_groups"][0]) == list(sd["param_groups"][0])  # the same keys before anything is loaded
    fresh_theirs = getattr(torch.optim, name)(torch_params(entries, torch.float32, with_grad=False))
    assert ours.state_dict()["param_groups"][0] == dict(fresh_theirs.state_dict()["param_groups"][0], lr=7e-3)
    ours.load_state_dict(copy.deepcopy(sd))
    mine = ours.state_dict()
    same_state(mine, sd)
    assert mine["state"][0]["step"].dtype == torch.float32 and mine["state"][0]["step"].dim() == 0
    assert mine["param_groups"][0]["params"] == list(range(len(entries))) and mine["param_groups"][0]["lr"] == 2e-3
    fresh_theirs.load_state_dict(copy.deepcopy(mine))
    same_state(fresh_theirs.state_dict(), sd)
    again = getattr(OPT, name)(torch_params(entries, torch.float32, with_grad=False))
    again.load_state_dict(copy.deepcopy(fresh_theirs.state_dict()))
    same_state(again.state_dict(), sd)
    # the loaded optimizers go on as the original does
    for q, r in zip(ps, fresh_theirs.param_groups[0]["params"]):
        r.data.copy_(q.data)
        r.grad = None if q.grad is None else q.grad.clone()
    theirs.step()
    fresh_theirs.step()
    assert all(torch.equal(q, r) for q, r in zip(ps, fresh_theirs.param_groups[0]["params"]))
    # assigning the learning rate (train.py:73) survives a round trip
    ours.param_groups[0]["lr"] = 5e-4
    other = getattr(OPT, name)(torch_params(entries, torch.float32, with_grad=False))
    other.load_state_dict(copy.deepcopy(ours.state_dict()))
    assert other.param_groups[0]["lr"] == 5e-4 and other.state_dict()["param_groups"][0]["lr"] == 5e-4
    # zero_grad as torch
    mine_ps = torch_params(entries, torch.float32)
    opt = getattr(OPT, name)(mine_ps)
    opt.zero_grad(set_to_none=False)
    assert all(q.grad is None or not q.grad.any() for q in mine_ps) and mine_ps[0].grad is not None
    opt.zero_grad()
    assert all(q.grad is None for q in mine_ps)


def test_refusals():
    ps = torch_params(R.main_list(CHUNK)[:3], torch.float32)
    with pytest.raises(NotImplementedError):
        OPT.Adam(ps, amsgrad=True)
    with pytest.raises(NotImplementedError):
        OPT.AdamW(ps, maximize=True)
    with pytest.raises(NotImplementedError):
        OPT.Adam([{"params": ps[:1]}, {"params": ps[1:], "lr": 1e-4}])
    with pytest.raises(NotImplementedError):
        OPT.clip_grad_norm_(ps, 1.0, norm_type=1)
    with pytest.raises(ValueError):
        OPT.Adam(ps, betas=(0.9, 1.0))
    opt = OPT.Adam(ps)
    before = [q.detach().clone() for q in ps]
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        opt.step()
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        opt.step(clip_norm=10.0)
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        OPT.clip_grad_norm_(ps, 1.0)
    assert all(torch.equal(a, b) for a, b in zip(before, ps)) and len(opt.state_dict()["state"]) == 0  # nothing moved, no state left
