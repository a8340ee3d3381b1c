"""GPU: the device optimizer -- pp_grad_norm / pp_scale_grads / pp_adam_step through the engine wrappers and framework.optim's
clip_grad_norm_, Adam and AdamW -- against numpy float64 (tests/optim_ref.py, pinned to torch's float64 run by test_optim_cpu.py).

Bars.  The norm: relative 2^-23, one fp32 rounding of the result plus a bit of slack (the fp64 accumulation error is far below it).
One step: the update dp = p_new - p_old, exp_avg and exp_avg_sq against the float64 step, each within 4 x ref32_dev x max |x64| over
the list, ref32_dev being the deviation of torch's own CPU float32 run of the same step from its float64 run, computed here.  The bar is
on dp, not on p: |p| is fifty steps large and would hide a wrong step.  Measured on an MI355X, the largest fraction of the bar over the
twelve cases of test_one_step: dp 0.25, exp_avg 0.25, exp_avg_sq 0.25 (the rounding of the stored values, which torch's float32 run
shares).  Everything else is equality of bits: two runs, a list against
its concatenation, clip against numpy's fp32 product, fused against unfused, resumed against uninterrupted."""
import copy

import numpy as np
import pytest
import torch

from conftest import load_pkg
import optim_ref as R
from test_blocktrain_gpu import GX, GY, dev, small_cfg, small_net, two_frames

pytestmark = pytest.mark.gpu
OPT = load_pkg("framework.optim")
CHUNK = load_pkg("_lib").PP_OPT_CHUNK
GROUP = load_pkg("_lib").PP_OPT_GROUP
VARIANTS = {"adam": ("Adam", 0.0), "adam_l2": ("Adam", 1e-2), "adamw": ("AdamW", 1e-2)}
LR = 1e-3
_ENG = []


def engine():
    if not _ENG:
        load_pkg().install()
        _ENG.append(load_pkg("engine").Engine(small_cfg(24, 16, 1)))
    return _ENG[0]


def place(a, kind):
    """A device tensor holding `a`; kind "view": one element into a larger buffer, so its address is 4-byte aligned only."""
    if kind != "view":
        return dev(a)
    buf = torch.zeros(a.size + 3, dtype=torch.float32, device="cuda")
    t = buf[1:1 + a.size]
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def params_of(entries, grads=True):
    ps = [torch.nn.Parameter(place(e["p"], e["kind"])) for e in entries]
    if grads:
        for q, e in zip(ps, entries):
            q.grad = None if e["g"] is None else place(e["g"], e["kind"])
    return ps


def inject(opt, entries, t):
    """State of a run that is about to take step t: exp_avg / exp_avg_sq from the entries and step = t - 1 for the parameters with a
    gradient; nothing at t = 1."""
    if t == 1:
        return
    sd = opt.state_dict()
    sd["state"] = {i: {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(e["m"].copy()), "exp_avg_sq": torch.from_numpy(e["v"].copy())}
                   for i, e in enumerate(entries) if e["g"] is not None}
    opt.load_state_dict(sd)


def torch_cpu_step(entries, t, name, wd, dtype):
    """torch's own optimizer on the CPU in `dtype`, one step from the entries' state -> per entry (p, m, v) float64 (None: no grad)."""
    ps = [torch.nn.Parameter(torch.from_numpy(e["p"].copy()).to(dtype)) for e in entries]
    for q, e in zip(ps, entries):
        q.grad = None if e["g"] is None else torch.from_numpy(e["g"].copy()).to(dtype)
    opt = getattr(torch.optim, name)(ps, lr=LR, weight_decay=wd)
    inject(opt, entries, t)
    opt.step()
    out = []
    for q, e in zip(ps, entries):
        st = opt.state[q]
        out.append(None if e["g"] is None else tuple(x.detach().double().numpy() for x in (q, st["exp_avg"], st["exp_avg_sq"])))
        assert e["g"] is None or int(st["step"]) == t
    return out


def bars(entries, t, name, wd):
    """-> (x64, bar, ref32_dev): per entry the float64 (dp, m, v) (None: no gradient or no elements), and per quantity the bar
    4 x ref32_dev x max |x64| over the list with torch's own float32 deviation ref32_dev."""
    r64, r32 = torch_cpu_step(entries, t, name, wd, torch.float64), torch_cpu_step(entries, t, name, wd, torch.float32)
    x64 = [None] * len(entries)
    dev32, top = np.zeros(3), np.zeros(3)
    for i, (e, a, b) in enumerate(zip(entries, r64, r32)):
        if a is None or e["p"].size == 0:
            continue
        p0 = e["p"].astype(np.float64)
        qa, qb = (a[0] - p0, a[1], a[2]), (b[0] - p0, b[1], b[2])
        x64[i] = qa
        for k in range(3):
            dev32[k] = max(dev32[k], np.abs(qb[k] - qa[k]).max())
            top[k] = max(top[k], np.abs(qa[k]).max())
    ref32_dev = dev32 / top
    return x64, 4.0 * ref32_dev * top, ref32_dev


def fractions(entries, ps, opt, x64, bar):
    """Largest |got - x64| per quantity over the list, as a fraction of the bar."""
    worst = np.zeros(3)
    for e, q, want in zip(entries, ps, x64):
        if want is None:
            continue
        st = opt.state[q]
        got = (q.detach().cpu().numpy().astype(np.float64) - e["p"].astype(np.float64), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy())
        for k in range(3):
            worst[k] = max(worst[k], np.abs(got[k] - want[k]).max())
    return worst / bar


def bits(ts):
    return [None if t is None else t.detach().clone() for t in ts]


def same_bits(a, b):
    return all((x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


# ------------------------------------------------------------------ 1. norm
def test_norm():
    eng = engine()
    for entries in (R.main_list(CHUNK), R.many_list()):
        with_g = [e for e in entries if e["g"] is not None]
        grads = [place(e["g"], e["kind"]) for e in with_g]
        a, b = eng.grad_norm(grads, 10.0), eng.grad_norm(grads, 10.0)
        assert a.shape == (2,) and a.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))
        want = R.total_norm([e["g"] for e in with_g])
        got = float(a[0])
        print(f"{len(grads)} tensors: norm {got:.9g}, float64 {want:.17g}, relative error {abs(got - want) / want:.2e} (bar {2.0 ** -23:.2e})")
        assert abs(got - want) <= 2.0 ** -23 * want
        assert float(a[1]) == 1.0  # 10 is above the norm
        half = eng.grad_norm(grads, 0.5 * want)
        assert half[0].item() == got and abs(float(half[1]) - R.clip_coef(want, 0.5 * want)) <= 4 * 2.0 ** -24
    many = R.many_list()
    assert len(many) > 2 * GROUP  # three launches
    one = eng.grad_norm([dev(np.concatenate([e["g"] for e in many]))], 10.0)
    lst = eng.grad_norm([dev(e["g"]) for e in many], 10.0)
    assert torch.equal(one.view(torch.int32), lst.view(torch.int32))
    # nothing to add: norm 0, coefficient 1 -- whatever max_norm is
    for grads in ([], [torch.zeros(0, device="cuda")], [torch.zeros((0, 3), device="cuda"), torch.zeros(0, device="cuda")]):
        assert eng.grad_norm(grads, 1e-9).tolist() == [0.0, 1.0]
    assert eng.grad_norm([torch.zeros(5, device="cuda")], 10.0).tolist() == [0.0, 1.0]


# ------------------------------------------------------------------ 2. clip
def test_clip():
    eng = engine()
    entries = R.main_list(CHUNK)
    want = R.total_norm([e["g"] for e in entries])
    ref = eng.grad_norm([dev(e["g"]) for e in entries if e["g"] is not None], 10.0)[0].item()
    # below the norm: every gradient is numpy's fp32 product with the coefficient read back
    ps = params_of(entries)
    norm = OPT.clip_grad_norm_(ps, 0.5 * want)
    assert norm.dim() == 0 and norm.dtype == torch.float32 and norm.is_cuda and norm.item() == ref
    coef = eng.grad_norm([dev(e["g"]) for e in entries if e["g"] is not None], 0.5 * want)[1].item()
    assert 0.49 < coef < 0.51
    for q, e in zip(ps, entries):
        if e["g"] is None:
            assert q.grad is None
            continue
        assert np.array_equal((e["g"] * np.float32(coef)).view(np.int32), q.grad.cpu().numpy().view(np.int32)), e["kind"]
    # above the norm: coefficient exactly 1, every bit unchanged (-0.0 and a denormal included)
    ps = params_of(entries)
    odd = np.array([-0.0, np.float32(1e-40)], np.float32)
    ps[2].grad[:2] = dev(odd)
    before = bits([q.grad for q in ps])
    assert OPT.clip_grad_norm_(ps, 10.0).item() == eng.grad_norm([g for g in before if g is not None], 10.0)[0].item()
    assert same_bits(before, [q.grad for q in ps])
    # one NaN: the norm is NaN and every gradient becomes NaN, as with torch
    ps = params_of(entries)
    ps[7].grad[5] = float("nan")
    theirs = [torch.nn.Parameter(q.detach().clone()) for q in ps]
    for r, q in zip(theirs, ps):
        r.grad = None if q.grad is None else q.grad.clone()
    with pytest.raises(RuntimeError, match="non-finite"):
        OPT.clip_grad_norm_(ps, 1.0, error_if_nonfinite=True)
    assert same_bits([r.grad for r in theirs], [q.grad for q in ps])  # raised before anything was scaled
    norm = OPT.clip_grad_norm_(ps, 1.0)
    tnorm = torch.nn.utils.clip_grad_norm_(theirs, 1.0)
    assert bool(torch.isnan(norm)) and bool(torch.isnan(tnorm))
    for q, r in zip(ps, theirs):
        if q.grad is not None:
            assert torch.equal(torch.isnan(q.grad), torch.isnan(r.grad)) and (q.grad.numel() == 0 or bool(torch.isnan(q.grad).all()))


# ------------------------------------------------------------------ 3. one step from arbitrary state
WORST = {}


@pytest.mark.parametrize("t", [1, 2, 10, 1000])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_one_step(variant, t):
    engine()
    name, wd = VARIANTS[variant]
    entries = R.main_list(CHUNK)
    if t == 1:
        entries = [dict(e, m=np.zeros_like(e["m"]), v=np.zeros_like(e["v"])) for e in entries]
    x64, bar, ref32_dev = bars(entries, t, name, wd)
    # the restatement is the float64 run
    for e, want in zip(entries, x64):
        if want is not None:
            p, m, v = R.adam_step(e["p"], e["g"], e["m"], e["v"], t, lr=LR, weight_decay=wd, decoupled=name == "AdamW")
            assert np.abs(p - e["p"] - want[0]).max() <= 1e-12 * np.abs(want[0]).max() + 1e-18
    ps = params_of(entries)
    opt = getattr(OPT, name)(ps, lr=LR, weight_decay=wd)
    inject(opt, entries, t)
    grads = bits([q.grad for q in ps])
    versions = [q._version for q in ps]
    assert opt.step() is None
    frac = fractions(entries, ps, opt, x64, bar)
    print(f"{variant} t={t}: ref32_dev dp {ref32_dev[0]:.2e} m {ref32_dev[1]:.2e} v {ref32_dev[2]:.2e}; "
          f"fraction of the bar: dp {frac[0]:.2f} m {frac[1]:.2f} v {frac[2]:.2f}")
    for k in range(3):
        WORST[k] = max(WORST.get(k, 0.0), frac[k])
    print("largest fractions so far: dp %.2f exp_avg %.2f exp_avg_sq %.2f" % tuple(WORST[k] for k in range(3)))
    assert (frac <= 1.0).all(), frac
    assert same_bits(grads, [q.grad for q in ps])  # g is not written
    for e, q, ver in zip(entries, ps, versions):
        if e["g"] is None:  # keeps its bits, gets no state, and its version does not move
            assert np.array_equal(q.detach().cpu().numpy().view(np.int32), e["p"].view(np.int32)) and q not in opt.state and q._version == ver
        else:
            assert float(opt.state[q]["step"]) == t and opt.state[q]["step"].dtype == torch.float32 and q._version > ver
            assert opt.state[q]["exp_avg"].shape == q.shape
    assert len(opt.state_dict()["state"]) == len(entries) - 1
    if t == 1000 and variant == "adam":
        # the test bites: a bias correction one step off misses the bar
        off = [R.adam_step(e["p"], e["g"], e["m"], e["v"], t + 1, lr=LR)[0] - e["p"] for e in entries if e["g"] is not None and e["p"].size]
        assert max(np.abs(o - w[0]).max() for o, w in zip(off, [w for w in x64 if w is not None])) > bar[0]


# ------------------------------------------------------------------ 4. fused equals unfused
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fused_equals_unfused(variant):
    engine()
    name, wd = VARIANTS[variant]
    entries = R.main_list(CHUNK) + R.many_list()[:40]
    norm = R.total_norm([e["g"] for e in entries])
    for c in (0.37 * norm, 10.0):
        runs = []
        for fused in (False, True):
            ps = params_of(entries)
            opt = getattr(OPT, name)(ps, lr=LR, weight_decay=wd)
            inject(opt, entries, 5)
            g0 = bits([q.grad for q in ps])
            if fused:
                n = opt.step(clip_norm=c)
                assert same_bits(g0, [q.grad for q in ps])  # the gradients keep their bits
            else:
                n = OPT.clip_grad_norm_(ps, c)
                opt.step()
                assert same_bits(g0, [q.grad for q in ps]) == (c > norm)
            runs.append([n.reshape(1)] + bits(ps) + bits([opt.state[q].get("exp_avg") for q in ps]) + bits([opt.state[q].get("exp_avg_sq") for q in ps]))
        assert same_bits(*runs)


# ------------------------------------------------------------------ 5. resume
def test_resume():
    engine()
    entries = R.main_list(CHUNK)

    def fresh():
        ps = params_of(entries)
        return ps, OPT.Adam(ps, lr=LR)

    ps_a, opt_a = fresh()
    for _ in range(3):
        opt_a.step(clip_norm=10.0)
    ps_b, opt_b = fresh()
    for _ in range(2):
        opt_b.step(clip_norm=10.0)
    sd = copy.deepcopy(opt_b.state_dict())
    mid = [q.detach().clone() for q in ps_b]
    ps_c = [torch.nn.Parameter(q.detach().clone()) for q in ps_b]
    for q, r in zip(ps_c, ps_b):
        q.grad = None if r.grad is None else r.grad.clone()
    opt_c = OPT.Adam(ps_c, lr=123.0)
    opt_c.load_state_dict(copy.deepcopy(sd))
    assert opt_c.param_groups[0]["lr"] == LR
    opt_c.step(clip_norm=10.0)
    for qa, qc in zip(ps_a, ps_c):
        assert torch.equal(qa.detach().view(torch.int32), qc.detach().view(torch.int32))
        if qa.grad is not None:
            sa, sc = opt_a.state[qa], opt_c.state[qc]
            assert float(sc["step"]) == 3.0 and float(sa["step"]) == 3.0
            assert all(torch.equal(sa[k].view(torch.int32), sc[k].view(torch.int32)) for k in ("exp_avg", "exp_avg_sq"))
    assert all(float(s["step"]) == 3.0 for s in opt_c.state_dict()["state"].values())
    # the same state in torch.optim.Adam on the GPU, one step: dp within twice the bar of test_one_step for this state
    ps_t = [torch.nn.Parameter(q.clone()) for q in mid]
    for q, r in zip(ps_t, ps_b):
        q.grad = None if r.grad is None else r.grad.clone()
    opt_t = torch.optim.Adam(ps_t, lr=55.0)
    opt_t.load_state_dict(copy.deepcopy(sd))
    opt_t.step()
    state = [dict(e, p=q.cpu().numpy(), m=sd["state"][i]["exp_avg"].cpu().numpy() if i in sd["state"] else e["m"],
                  v=sd["state"][i]["exp_avg_sq"].cpu().numpy() if i in sd["state"] else e["v"]) for i, (e, q) in enumerate(zip(entries, mid))]
    _, bar, _ = bars(state, 3, "Adam", 0.0)
    worst = 0.0
    for q0, qt, qc in zip(mid, ps_t, ps_c):
        if q0.numel():
            worst = max(worst, float(((qt.detach().double() - q0.double()) - (qc.detach().double() - q0.double())).abs().max()))
    print(f"torch.optim.Adam resumed from our state: dp differs by {worst:.3e}, bar {2 * bar[0]:.3e} ({worst / (2 * bar[0]):.2f} of it)")
    assert worst <= 2 * bar[0]
    assert all(float(opt_t.state[q]["step"]) == 3.0 for q in ps_t if q.grad is not None)


# ------------------------------------------------------------------ 6. through the network
def fixed_batch(eng):
    rng = np.random.default_rng(21)
    u = rng.random((2, eng.A))
    labels = np.where(u < 1 / 7, 1, np.where(u < 0.75, 0, -1)).astype(np.int32)
    return {"labels": labels, "bbox_targets": (rng.standard_normal((2, eng.A, 7)) * 0.4).astype(np.float32) * (labels > 0)[..., None],
            "dir_targets": (rng.random((2, eng.A)) < 0.5).astype(np.int32)}


def test_through_the_network():
    load_pkg().install()
    shared = load_pkg("networks.pointpillars8_shared")
    lg_cls = load_pkg("framework.loss_generator").LossGenerator
    net, cfg = small_net()
    eng = net._eng
    example, ex = two_frames(eng), fixed_batch(eng)
    lg = lg_cls(cfg)
    net.train(scope="all")
    named = list(net.named_parameters())
    assert [k for k, _ in named] == list(shared.ALL_KEYS) and len(named) == 28
    opt = OPT.Adam(net.parameters(), lr=LR)
    loss = lg.generate(net(example), ex)["loss"]
    opt.zero_grad()
    loss.backward()
    entries = [dict(p=q.detach().cpu().numpy().reshape(-1), g=q.grad.cpu().numpy().reshape(-1), m=np.zeros(q.numel(), np.float32),
                    v=np.zeros(q.numel(), np.float32), kind="plain") for _, q in named]
    want = R.total_norm([e["g"] for e in entries])
    norm = OPT.clip_grad_norm_(net.parameters(), 10.0)
    print(f"28 gradients: norm {float(norm):.9g}, float64 {want:.17g}, relative error {abs(float(norm) - want) / want:.2e}")
    assert abs(float(norm) - want) <= 2.0 ** -23 * want
    clipped = [dict(e, g=q.grad.cpu().numpy().reshape(-1)) for e, (_, q) in zip(entries, named)]
    x64, bar, _ = bars(clipped, 1, "Adam", 0.0)
    opt.step()
    flat = [q.detach().reshape(-1) for _, q in named]
    worst = np.zeros(3)
    for e, q, (_, par), w in zip(clipped, flat, named, x64):
        st = opt.state[par]
        got = (q.cpu().numpy().astype(np.float64) - e["p"], st["exp_avg"].cpu().numpy().reshape(-1), st["exp_avg_sq"].cpu().numpy().reshape(-1))
        worst = np.maximum(worst, [np.abs(got[k] - w[k]).max() for k in range(3)])
    print("network step, fraction of the bar: dp %.2f exp_avg %.2f exp_avg_sq %.2f" % tuple(worst / bar))
    assert (worst <= bar).all(), worst / bar
    # twenty fused steps on the fixed batch
    losses = [float(loss.detach())]
    for _ in range(20):
        opt.zero_grad()
        loss = lg.generate(net(example), ex)["loss"]
        loss.backward()
        n = opt.step(clip_norm=10.0)
        losses.append(float(loss.detach()))
        assert n.dim() == 0 and n.is_cuda
    with torch.no_grad():
        losses.append(float(lg.generate(net(example), ex)["loss"]))
    print("all", " ".join(f"{v:.6f}" for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert all(float(s["step"]) == 21.0 for s in opt.state_dict()["state"].values())
    # every packed image was rewritten: a fresh network loaded from state_dict() computes the same bits
    net.eval()
    other, _ = small_net()
    other.load_state_dict(net.state_dict())
    pa, pb = net(example), other(example)
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    rng = np.random.default_rng(5)
    pts = dev(rng.uniform([0, 0, -1.5, 0], [0.2 * GX, 0.2 * GY, 1.0, 1], (3000, 4)).astype(np.float32))
    da, db = eng.infer_frame(pts), other._eng.infer_frame(pts)
    assert torch.equal(eng.fetch(0, "rpn"), other._eng.fetch(0, "rpn")) and all(torch.equal(x, y) for x, y in zip(da, db))


def test_head_scope():
    load_pkg().install()
    shared = load_pkg("networks.pointpillars8_shared")
    net, cfg = small_net()
    eng = net._eng
    example, ex = two_frames(eng), fixed_batch(eng)
    lg = load_pkg("framework.loss_generator").LossGenerator(cfg)
    start = {k: np.array(v, copy=True) for k, v in net.state_dict().items()}
    net.train(scope="head")
    assert len(list(net.parameters())) == 6
    opt = OPT.AdamW(net.parameters(), lr=LR)
    for _ in range(3):
        opt.zero_grad()
        lg.generate(net(example), ex)["loss"].backward()
        opt.step(clip_norm=10.0)
    net.eval()
    end = net.state_dict()
    for k in start:
        moved = np.abs(np.asarray(end[k], np.float64) - np.asarray(start[k], np.float64).reshape(np.shape(end[k]))).max() > 0
        assert moved == (k in shared.HEAD_KEYS), k
    other, _ = small_net()
    other.load_state_dict(end)
    pa, pb = net(example), other(example)
    assert all(torch.equal(pa[k], pb[k]) for k in pa)


# ------------------------------------------------------------------ 7. refusals
def test_refusals():
    eng = engine()
    entries = R.main_list(CHUNK)[:7]

    def run():
        ps = params_of(entries)
        m, v = [dev(e["m"]) for e in entries], [dev(e["v"]) for e in entries]
        eng.adam_step(ps, [q.grad for q in ps], m, v, 4, LR, 0.9, 0.999, 1e-8)
        return bits(ps) + m + v + [eng.grad_norm([q.grad for q in ps], 1.0)]

    base = run()
    ps = params_of(entries)
    g, m, v = [q.grad for q in ps], [dev(e["m"]) for e in entries], [dev(e["v"]) for e in entries]
    keep = bits(ps) + bits(m) + bits(v)

    def swapped(lst, i, t):
        return lst[:i] + [t] + lst[i + 1:]

    wide = torch.zeros((576, 2), device="cuda")[:, 0]
    assert not wide.is_contiguous()
    args = (4, LR, 0.9, 0.999, 1e-8)
    with pytest.raises(TypeError):
        eng.adam_step(swapped(ps, 5, ps[5].detach().cpu()), g, m, v, *args)
    with pytest.raises(TypeError):
        eng.adam_step(ps, swapped(g, 5, g[5].double()), m, v, *args)
    with pytest.raises(ValueError):
        eng.adam_step(swapped(ps, 5, wide), g, m, v, *args)
    with pytest.raises(ValueError):
        eng.adam_step(ps, g, swapped(m, 5, torch.zeros(575, device="cuda")), v, *args)
    with pytest.raises(ValueError):
        eng.adam_step(ps, g, m, v, 0, *args[1:])
    with pytest.raises(RuntimeError, match="beta"):
        eng.adam_step(ps, g, m, v, 4, LR, 1.0, 0.999, 1e-8)
    with pytest.raises(TypeError):
        eng.grad_norm(swapped(g, 1, g[1].cpu()), 1.0)
    with pytest.raises(TypeError):
        eng.scale_grads(g, torch.ones(1))
    with pytest.raises(ValueError):
        eng.scale_grads(swapped(g, 5, wide), torch.ones(1, device="cuda"))
    assert same_bits(keep, bits(ps) + m + v)  # nothing ran
    # the optimizer refuses the same before anything runs, and leaves no state behind
    bad = params_of(entries)
    bad[5] = torch.nn.Parameter(torch.zeros((576, 2), device="cuda").t())
    bad[5].grad = torch.zeros((576, 2), device="cuda").t()
    opt = OPT.Adam(bad)
    was = bits(bad)
    with pytest.raises(ValueError):
        opt.step(clip_norm=1.0)
    assert same_bits(was, bits(bad)) and len(opt.state_dict()["state"]) == 0
    assert same_bits(base, run())  # the call that follows gives the bits it gave before
