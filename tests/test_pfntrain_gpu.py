"""GPU: training the pillar feature net -- PointNet in train mode with its arg (pp_pfn_train_forward), the scatter's backward
(pp_scatter_backward), the closed-form PFN backward (pp_pfn_backward), the in-place update of the eval-mode PFN (pp_update_pfn_weights)
and the autograd surface PointPillars.train(scope="all") -- against the reference's float64 autograd goldens
(tests/golden/make_pfntrain_goldens.py) and the float64 restatement pinned to them (tests/pfntrain_ref.py).

Bars.  Fixture values and gradients: 4 x ref32_dev x max |x64| per tensor, ref32_dev being the reference's own float32-against-float64
deviation stored in the fixture (the project's margin, train_common.check_grad).  The fixture's seed keeps every argmax and ReLU
decision 2^-15 away from a tie, so arg is compared exactly.  At 5000 pillars near-ties cannot be excluded: there the GPU's selection
must maximise the float64 activations to within 1e-5, and the gradients are compared, at case a's bars (same pillar geometry), with the
restatement evaluated at the GPU's own selection and ReLU branches.  Equality is asserted between two runs, between the autograd
surface and the same chain made by hand with the engine primitives, between scopes on the tensors they share, and between an engine
whose PFN was rewritten in place and a fresh engine that committed the same values."""
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden, load_pkg
import pfntrain_ref as R
from train_common import GX, GY, by_hand, canvases_of, dev, seeded_sd, small_cfg, small_net, stacked_taps, two_frames  # noqa: F401

sys.path.insert(0, GOLDEN)
import make_pfntrain_goldens as G  # noqa: E402

pytestmark = pytest.mark.gpu
ENG = load_pkg("engine").Engine
PFN, STAT = ENG.PFN_KEYS, ENG.PFN_STAT_KEYS
_ENGINES = {}


def engine(T, max_voxels=2000, max_batch=2):
    """An engine without weights on the fixture's geometry (the PFN training entry points are stateless)."""
    key = (T, max_voxels, max_batch)
    if key not in _ENGINES:
        load_pkg().install()
        cfg = small_cfg(G.GX, G.GY, max_batch)
        cfg["max_num_points"], cfg["max_voxels"] = T, max_voxels
        eng = _ENGINES[key] = ENG(cfg)
        vx, vy, xo, yo = G.geometry()
        assert eng.T == T and tuple(eng.grid_size[:2]) == (G.GX, G.GY)
        assert eng.voxel_size[0] == vx and eng.voxel_size[1] == vy and eng.voxel_size[0] / 2 + eng.offset[0] == xo and \
            eng.voxel_size[1] / 2 + eng.offset[1] == yo  # the restatement's geometry is the engine's
    return _ENGINES[key]


def on_device(inp):
    return {k: dev(v) for k, v in inp.items()}


def check(got, want64, ref32_dev, what):
    got = got.cpu().numpy().astype(np.float64).reshape(-1)
    bar = 4.0 * ref32_dev * np.abs(want64).max()
    err = np.abs(got - np.asarray(want64).reshape(-1)).max()
    print(f"{what}: max err {err:.3e}, bar {bar:.3e} ({err / bar:.2f} of it)")
    return err <= bar


def forward_of(eng, d):
    num = eng.num_tensor(d["voxels"].shape[0])
    return num, eng.pfn_train_forward(d["voxels"], d["coors"], d["npts"], num, d["w"], d["gamma"], d["beta"])


# ------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("case", list(G.CASES))
def test_forward(case):
    g = golden("pfntrain_small")
    d = on_device(G.small_inputs(case))
    eng = engine(G.CASES[case]["T"])
    _, (feat, arg, stats) = forward_of(eng, d)
    assert feat.shape == arg.shape == (d["voxels"].shape[0], 64) and stats.shape == (218,) and stats.dtype == torch.float64
    assert np.array_equal(arg.cpu().numpy(), g["arg_" + case])
    ok = [check(feat, g["feat_" + case], float(g[f"ref32_dev_feat_{case}"]), f"{case} feat"),
          check(stats[:64], g["mean_" + case], float(g[f"ref32_dev_mean_{case}"]), f"{case} mean"),
          check(stats[64:128], g["var_" + case], float(g[f"ref32_dev_var_{case}"]), f"{case} var")]
    assert all(ok), ok
    # s and M are what the restatement sums, and M is symmetric
    inp = G.small_inputs(case)
    fwd = R.forward(R.features(inp["voxels"], inp["coors"], inp["npts"], *G.geometry()), inp["w"], inp["gamma"], inp["beta"])
    s, M = stats[128:137].cpu().numpy(), stats[137:].cpu().numpy().reshape(9, 9)
    assert np.array_equal(M, M.T)
    assert np.abs(s - fwd["s"]).max() <= 1e-6 * np.abs(fwd["s"]).max() and np.abs(M - fwd["M"]).max() <= 1e-6 * np.abs(fwd["M"]).max()


# ------------------------------------------------------------------ 2. backward
@pytest.mark.parametrize("case", list(G.CASES))
def test_backward(case):
    g = golden("pfntrain_small")
    d = on_device(G.small_inputs(case))
    eng = engine(G.CASES[case]["T"])
    num, (feat, arg, stats) = forward_of(eng, d)
    dw, dg, db = eng.pfn_backward(d["voxels"], d["coors"], d["npts"], num, d["w"], d["gamma"], stats, feat, arg, d["g"])
    assert dw.shape == (64, 9, 1) and dg.shape == db.shape == (64,)
    ok = [check(t, g[f"{k}_{case}"], float(g[f"ref32_dev_{k}_{case}"]), f"{case} {k}") for k, t in (("dw", dw), ("dgamma", dg), ("dbeta", db))]
    assert all(ok), ok


# ------------------------------------------------------------------ 3. scatter backward
def test_scatter_backward():
    eng = engine(15)
    rng = np.random.default_rng(2)
    n = 301
    cells = rng.choice(G.GX * G.GY, n, replace=False)
    coors = np.stack([cells // G.GY, cells % G.GY, np.zeros(n, np.int64)], 1).astype(np.int32)
    coors[7] = (G.GX, 3, 0)  # outside the grid: the forward skips it
    dcanvas = rng.standard_normal((1, 64, G.GX, G.GY)).astype(np.float32)
    dc, c = dev(dcanvas), dev(coors)
    got = eng.scatter_backward(dc, c, eng.num_tensor(n))
    inside = torch.ones(n, dtype=torch.bool, device="cuda")
    inside[7] = False
    idx = (c[:, 0].long() * G.GY + c[:, 1].long()).clamp(0, G.GX * G.GY - 1)
    want = dc.reshape(64, -1)[:, idx].t() * inside[:, None]
    assert got.shape == (n, 64) and torch.equal(got, want.contiguous())
    assert not got[7].any() and got[6].any()
    # it is the backward of scatter: <scatter(feat), dcanvas> = <feat, scatter_backward(dcanvas)> on the pillars inside the grid
    feat = dev(rng.standard_normal((n, 64)).astype(np.float32))
    lhs = (eng.scatter(feat, c, eng.num_tensor(n)).double() * dc.double()).sum()
    rhs = (feat.double() * got.double()).sum()
    assert abs(float(lhs - rhs)) <= 1e-9 * abs(float(lhs))
    # into the rows of a larger tensor, and fewer pillars than rows
    big = torch.full((n + 5, 64), 7.0, device="cuda")
    eng.scatter_backward(dc, c, eng.num_tensor(n - 1), out=big[2:2 + n])
    assert torch.equal(big[2:1 + n], want[:n - 1]) and bool((big[:2] == 7).all()) and bool((big[1 + n:] == 7).all())


# ------------------------------------------------------------------ 4. large P
def test_large_batch_of_pillars():
    """5000 pillars at T = 15 on an engine with max_voxels 2600 and max_batch 2: more pillars than either pass has waves, so the
    grid-stride loops and both reduction stages run more than once."""
    g = golden("pfntrain_small")
    eng = engine(15, max_voxels=2600, max_batch=2)
    T, P = 15, 5000
    rng = np.random.default_rng(31)
    cells = rng.integers(0, G.GX * G.GY, P)
    coors = np.stack([cells // G.GY, cells % G.GY, np.zeros(P, np.int64)], 1).astype(np.int32)
    npts = rng.integers(1, T + 1, P).astype(np.int32)
    u = rng.random((P, T, 4))
    vox = np.stack([(coors[:, None, 0] + u[:, :, 0]) * 0.2, (coors[:, None, 1] + u[:, :, 1]) * 0.2, u[:, :, 2] * 3.0 - 2.0, u[:, :, 3]], -1)
    vox = (vox * (np.arange(T)[None, :] < npts[:, None])[:, :, None]).astype(np.float32)
    small = G.small_inputs("a")
    inp = dict(voxels=vox, coors=coors, npts=npts, w=small["w"], gamma=small["gamma"], beta=small["beta"], g=rng.standard_normal((P, 64)).astype(np.float32))
    d = on_device(inp)
    runs = []
    for _ in range(2):
        num, (feat, arg, stats) = forward_of(eng, d)
        grads = eng.pfn_backward(d["voxels"], d["coors"], d["npts"], num, d["w"], d["gamma"], stats, feat, arg, d["g"])
        runs.append((feat, arg, stats) + tuple(grads))
    assert all(torch.equal(a, b) for a, b in zip(*runs))  # fixed-order sums: bit for bit
    feat, arg, stats, dw, dg, db = runs[0]
    f = R.features(vox, coors, npts, *G.geometry())
    fwd = R.forward(f, inp["w"], inp["gamma"], inp["beta"])
    ga, gf = arg.cpu().numpy(), feat.cpu().numpy()
    slack = R.maximiser_slack(fwd["y"], ga)
    print(f"args that differ from the float64 argmax: {int((ga != fwd['arg']).sum())} of {ga.size}, largest slack {slack.max():.3e}; "
          f"ReLU branches that differ: {int(((gf > 0) != (fwd['feat'] > 0)).sum())}")
    assert slack.max() <= 1e-5
    ok = [check(feat, fwd["feat"], float(g["ref32_dev_feat_a"]), "large feat"),
          check(stats[:64], fwd["mean"], float(g["ref32_dev_mean_a"]), "large mean"),
          check(stats[64:128], fwd["var"], float(g["ref32_dev_var_a"]), "large var")]
    want = R.backward(f, inp["w"], inp["gamma"], dict(fwd, feat=gf), inp["g"], arg=ga)
    ok += [check(t, w64, float(g[f"ref32_dev_{k}_a"]), f"large {k}") for (k, t), w64 in zip((("dw", dw), ("dgamma", dg), ("dbeta", db)), want)]
    assert all(ok), ok


# ------------------------------------------------------------------ 5. weight update
def test_update_pfn_weights():
    load_pkg().install()
    sd = seeded_sd()
    eng = ENG(small_cfg(GX, GY, 2))
    eng.load_state_dict(sd)
    rng = np.random.default_rng(6)
    new = dict(sd)
    for k in PFN + STAT[:1]:
        new[k] = sd[k] + rng.standard_normal(sd[k].shape).astype(np.float32) * np.float32(0.05)
    new[STAT[1]] = sd[STAT[1]] * rng.uniform(0.5, 1.5, 64).astype(np.float32)
    fresh = ENG(small_cfg(GX, GY, 2))
    fresh.load_state_dict(new)
    n = 400
    cells = rng.choice(GX * GY, n, replace=False)
    c = dev(np.stack([cells // GY, cells % GY, np.zeros(n, np.int64)], 1).astype(np.int32))
    v = dev(rng.standard_normal((n, eng.T, 4)).astype(np.float32))
    k = dev(rng.integers(1, eng.T + 1, n).astype(np.int32))
    pts = dev(rng.uniform([0, 0, -1.5, 0], [0.2 * GX, 0.2 * GY, 1.0, 1], (3000, 4)).astype(np.float32))

    def outputs(e):
        feat = e.pfn(v, c, k, e.num_tensor(n)).clone()
        det, cnt = e.infer_frame(pts)
        return feat, e.fetch(0, "rpn").clone(), det.clone(), cnt.clone()

    want = {"old": outputs(eng), "new": outputs(fresh)}
    assert (want["old"][0] - want["new"][0]).abs().max() > 1e-3 and (want["old"][1] - want["new"][1]).abs().max() > 1e-4
    for which, vals in (("new", new), ("old", sd)):  # perturbed values, and back: the weights are restored
        eng.update_pfn_weights(*[dev(vals[key]) for key in PFN + STAT])
        got = outputs(eng)
        assert all(torch.equal(a, b) for a, b in zip(got, want[which])), which
    empty = ENG(small_cfg(GX, GY, 2))
    with pytest.raises(RuntimeError, match="not committed"):
        empty.update_pfn_weights(*[dev(sd[key]) for key in PFN + STAT])
    with pytest.raises(ValueError):
        eng.update_pfn_weights(*[dev(sd[key]) for key in PFN + STAT[:1]], dev(sd[STAT[1]])[:-1])


# ------------------------------------------------------------------ 6. autograd surface
def frames_of(example):
    coors = example["coordinates"]
    out = []
    for f in range(2):
        sel = coors[:, -1] == f
        out.append((example["voxels"][sel].contiguous(), coors[sel][:, :-1].contiguous(), example["num_points_per_voxel"][sel].contiguous()))
    return out


def restated_stats(eng, frames, p):
    vs, off = eng.voxel_size, eng.offset
    v, c, n = (torch.cat([f[i] for f in frames]).cpu().numpy() for i in range(3))
    f = R.features(v, c, n, vs[0], vs[1], vs[0] / np.float32(2) + off[0], vs[1] / np.float32(2) + off[1])
    return R.forward(f, *[p[k].detach().cpu().numpy() for k in PFN])


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def test_autograd_surface():
    load_pkg().install()
    net, _ = small_net()
    eng = net._eng
    shared = load_pkg("networks.pointpillars8_shared")
    example = two_frames(eng)
    frames = frames_of(example)
    sd0 = net.state_dict()
    net.train(scope="all")
    names = [k for k, _ in net.named_parameters()]
    assert names == list(shared.ALL_KEYS) and len(names) == 28 and all(p.is_cuda and p.requires_grad for p in net.parameters())
    p = {k: v.detach().clone() for k, v in net.named_parameters()}
    preds = net(example)
    rng = np.random.default_rng(8)
    up = {k: dev(rng.standard_normal(tuple(v.shape)).astype(np.float32) * np.float32(1e-2)) for k, v in preds.items()}
    net.zero_grad()
    sum((preds[k] * up[k]).sum() for k in preds).backward()
    grads = {k: q.grad.clone() for k, q in net.named_parameters()}
    # the running statistics after one forward, against the restatement
    fwd = restated_stats(eng, frames, p)
    rm, rv = R.running(sd0[STAT[0]], sd0[STAT[1]], fwd)
    sd1 = net.state_dict()
    print("running_mean", rel(sd1[STAT[0]], rm), "running_var", rel(sd1[STAT[1]], rv))
    assert rel(sd1[STAT[0]], rm) <= 1e-6 and rel(sd1[STAT[1]], rv) <= 1e-6
    assert np.abs(sd1[STAT[0]] - sd0[STAT[0]]).max() > 1e-3
    # the same chain by hand with the engine primitives
    v, c, n = (torch.cat([f[i] for f in frames]) for i in range(3))
    num = eng.num_tensor(v.shape[0])
    feat, arg, stats = eng.pfn_train_forward(v, c, n, num, *[p[k] for k in PFN])
    rows = np.cumsum([0] + [f[0].shape[0] for f in frames])
    nums = [eng.num_tensor(f[0].shape[0]) for f in frames]
    canvases = torch.cat([eng.scatter(feat[rows[i]:rows[i + 1]], frames[i][1], nums[i]) for i in range(2)])
    taps = stacked_taps(eng, list(canvases.split(1)))
    y = taps[0]
    gh, dxh = eng.head_backward(y, up["cls_preds"], up["box_preds"], up["dir_preds"])
    for k in shared.HEAD_KEYS:
        assert torch.equal(grads[k], gh[k].reshape(p[k].shape)), k
    dw, dcanvas, _ = by_hand(eng, canvases, taps, p, dxh, need_dx=True)
    dfeat = torch.cat([eng.scatter_backward(dcanvas[i:i + 1].contiguous(), frames[i][1], nums[i]) for i in range(2)])
    hand = eng.pfn_backward(v, c, n, num, p[PFN[0]], p[PFN[1]], stats, feat, arg, dfeat)
    for k, t in zip(PFN, hand):
        assert torch.equal(grads[k], t) and float(t.abs().max()) > 0, k
    # the 25 tensors behind the canvases: a run that feeds rpn_train the same canvases under scope "rpn"
    net.train(scope="rpn")
    net.zero_grad()
    out = net.heads(net.rpn_train(canvases))
    assert all(torch.equal(out[k].detach(), preds[k].detach()) for k in preds)
    sum((out[k] * up[k]).sum() for k in out).backward()
    rpn = {k: q.grad for k, q in net.named_parameters()}
    assert list(rpn) == list(shared.RPN_KEYS)
    for k in shared.RPN_KEYS:
        assert torch.equal(grads[k], rpn[k]) and torch.equal(grads[k], dw[k] if k in dw else gh[k].reshape(p[k].shape)), k
    assert all(q.grad is None for q in net._pfn.values())
    # without grad the training forward still moves the running statistics, as BatchNorm1d does; eval() does not
    net.train(scope="all")
    with torch.no_grad():
        again = net(example)
    assert all(v.grad_fn is None for v in again.values()) and all(torch.equal(again[k], preds[k].detach()) for k in preds)
    sd2 = net.state_dict()
    rm2, rv2 = R.running(rm, rv, fwd)
    assert rel(sd2[STAT[0]], rm2) <= 1e-6 and rel(sd2[STAT[1]], rv2) <= 1e-6


# ------------------------------------------------------------------ 7. trajectory
def test_trajectory():
    """Three Adam steps on a fixed batch of two frames under scope "all": the loss falls, all 28 tensors and the running statistics
    move, and after eval() the network is the one a fresh object loads from state_dict()."""
    load_pkg().install()
    shared = load_pkg("networks.pointpillars8_shared")
    LossGenerator = load_pkg("framework.loss_generator").LossGenerator
    net, cfg = small_net()
    eng = net._eng
    example = two_frames(eng)
    rng = np.random.default_rng(21)
    u = rng.random((2, eng.A))
    labels = np.where(u < 1 / 7, 1, np.where(u < 0.75, 0, -1)).astype(np.int32)
    ex = {"labels": labels, "bbox_targets": (rng.standard_normal((2, eng.A, 7)) * 0.4).astype(np.float32) * (labels > 0)[..., None],
          "dir_targets": (rng.random((2, eng.A)) < 0.5).astype(np.int32)}
    lg = LossGenerator(cfg)
    sd = dict(net.state_dict())
    sd[shared.PFN_NBT_KEY] = np.asarray(0, np.int64)
    net.load_state_dict(sd)
    start = {k: np.array(v, copy=True) for k, v in net.state_dict().items()}
    net.train(scope="all")
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    losses = []
    for _ in range(3):
        loss = lg.generate(net(example), ex)["loss"]
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(lg.generate(net(example), ex)["loss"]))
    print("all", " ".join(f"{v:.6f}" for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    net.eval()
    end = net.state_dict()
    for k in shared.ALL_KEYS + STAT:
        assert np.abs(end[k] - np.asarray(start[k], np.float32).reshape(end[k].shape)).max() > 1e-5, k
    assert int(end[shared.PFN_NBT_KEY]) == 4 and end[shared.PFN_NBT_KEY].dtype == np.int64
    other, _ = small_net()
    other.load_state_dict(end)
    pa, pb = net(example), other(example)
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    pts = dev(rng.uniform([0, 0, -1.5, 0], [0.2 * GX, 0.2 * GY, 1.0, 1], (3000, 4)).astype(np.float32))
    da, db = eng.infer_frame(pts), other._eng.infer_frame(pts)  # the fused pass reads the same PFN buffers
    assert torch.equal(eng.fetch(0, "rpn"), other._eng.fetch(0, "rpn")) and all(torch.equal(x, y) for x, y in zip(da, db))
    net(example)  # a second eval forward
    after = net.state_dict()
    assert all(np.array_equal(after[k], end[k]) for k in STAT + (shared.PFN_NBT_KEY,))


def test_rpn_scope_is_unchanged():
    """Scope "rpn" on a freshly loaded network: the forward is the inference forward and the gradients are those of the chain made by
    hand from the frozen eval-mode PFN's canvases (train_common.by_hand): the code path of the scopes that existed before."""
    load_pkg().install()
    shared = load_pkg("networks.pointpillars8_shared")
    net, _ = small_net()
    eng = net._eng
    example = two_frames(eng)
    plain = net(example)
    sd0 = net.state_dict()
    net.train(scope="rpn")
    preds = net(example)
    assert all(torch.equal(preds[k].detach(), plain[k]) for k in plain)
    rng = np.random.default_rng(8)
    up = {k: dev(rng.standard_normal(tuple(v.shape)).astype(np.float32) * np.float32(1e-2)) for k, v in plain.items()}
    net.zero_grad()
    sum((preds[k] * up[k]).sum() for k in preds).backward()
    p = {k: v.detach() for k, v in net.named_parameters()}
    assert list(p) == list(shared.RPN_KEYS)
    frames = canvases_of(eng, example)
    canvases = torch.cat(frames)
    taps = stacked_taps(eng, frames)
    gh, dxh = eng.head_backward(taps[0], up["cls_preds"], up["box_preds"], up["dir_preds"])
    dw, _, _ = by_hand(eng, canvases, taps, p, dxh, need_dx=False)
    for k, q in net.named_parameters():
        assert torch.equal(q.grad, dw[k] if k in dw else gh[k].reshape(q.shape)), k
    sd1 = net.state_dict()
    assert all(np.array_equal(sd1[k], sd0[k]) for k in PFN + STAT) and all(q.grad is None for q in net._pfn.values())


# ------------------------------------------------------------------ 8. refusals
def test_refusals():
    load_pkg().install()
    d = on_device(G.small_inputs("a"))
    eng = engine(15)
    base = forward_of(eng, d)[1]
    none = [t[:0].contiguous() for t in (d["voxels"], d["coors"], d["npts"])]
    with pytest.raises(RuntimeError, match="pillars x max_num_points < 2"):  # P T < 2: no unbiased variance
        eng.pfn_train_forward(*none, eng.num_tensor(0), d["w"], d["gamma"], d["beta"])
    with pytest.raises(RuntimeError, match="pillars x max_num_points < 2"):  # the count on the device decides, not the rows
        eng.pfn_train_forward(d["voxels"], d["coors"], d["npts"], eng.num_tensor(0), d["w"], d["gamma"], d["beta"])
    wide = engine(256)
    v = torch.zeros((3, 256, 4), device="cuda")
    with pytest.raises(RuntimeError, match="255"):
        wide.pfn_train_forward(v, d["coors"][:3].contiguous(), d["npts"][:3].contiguous(), wide.num_tensor(3), d["w"], d["gamma"], d["beta"])
    with pytest.raises(ValueError):
        eng.pfn_train_forward(d["voxels"][:, :-1].contiguous(), d["coors"], d["npts"], eng.num_tensor(3), d["w"], d["gamma"], d["beta"])
    with pytest.raises(TypeError):
        eng.pfn_train_forward(d["voxels"].cpu(), d["coors"], d["npts"], eng.num_tensor(3), d["w"], d["gamma"], d["beta"])
    with pytest.raises(ValueError):
        eng.pfn_backward(d["voxels"], d["coors"], d["npts"], eng.num_tensor(3), d["w"], d["gamma"], base[2], base[0], base[1], d["g"][:-1])
    assert all(torch.equal(a, b) for a, b in zip(forward_of(eng, d)[1], base))  # the next call works
    # the autograd surface in a 16-bit mode
    net, _ = small_net()
    example = two_frames(net._eng)
    net.train(scope="all")
    good = net(example)
    sd = net.state_dict()
    net.half()
    with pytest.raises(RuntimeError, match="fp32"):
        net(example)
    assert all(np.array_equal(net.state_dict()[k], sd[k]) for k in STAT)  # refused before the running statistics moved
    net.float()
    again = net(example)
    assert all(again[k].requires_grad and torch.equal(again[k].detach(), good[k].detach()) for k in good)
    with pytest.raises(ValueError, match="'all'"):
        net.train(scope="bogus")
