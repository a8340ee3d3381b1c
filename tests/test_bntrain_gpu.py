"""GPU: fine-tuning the BatchNorm network with frozen statistics -- the three affine backward primitives (pp_unit_backward_affine,
pp_down_backward_affine, pp_neck_backward_affine), the fold on the device (pp_bn_fold, pp_update_bn_fold, pp_bn_affine_grad) and the
autograd surface PointPillars.train(scope=..., bn_stats="frozen") of networks.pointpillars8_export -- against the float64 restatement
(tests/bntrain_ref.py) and the reference's float64 autograd goldens (tests/golden/make_bntrain_goldens.py).

Bars.  Primitives: the element-wise a-priori bounds of bntrain_ref (float32 summation in any order from the same float32 inputs; the
affine norm's ReLU mask is exact, so there are no near-ties to set aside).  Fixture gradients: 4 x ref32_dev x max |g64| per tensor,
the bar of test_rpntrain_gpu.py.  Equality is asserted between identical calls, with and without du / dx, for a frame whatever batch
it rides in, for the dskip add, between rpn_train() and rpn(), and between an engine whose fold was rewritten in place and a fresh
engine that committed the same values."""
import ctypes
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden, load_pkg
import bntrain_ref as R
from train_common import GX, GY, canvases_of, check_bound, check_grad, dev, engine, small_cfg, two_frames

sys.path.insert(0, GOLDEN)
from make_bntrain_goldens import DW_STRIDE, DX_STRIDE, small_inputs, split  # noqa: E402

pytestmark = pytest.mark.gpu
ENG = load_pkg("engine").Engine
BAR = 2e-4  # the project's backbone bar


def norm_params(rng, C):
    return (rng.uniform(0.5, 1.5, C).astype(np.float32), (rng.standard_normal(C) * 0.1).astype(np.float32),
            (rng.standard_normal(C) * 0.1).astype(np.float32), rng.uniform(0.5, 1.5, C).astype(np.float32))


def check_all(got, want, bounds, what):
    for name, g, w, b in zip(("dw", "dx", "dscale", "dshift"), got, want, bounds):
        assert g.dtype == (torch.float64 if name[1] == "s" else torch.float32), name
        check_bound(g, w, b, f"{what} {name}")


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def bn_sd(seed=0):
    return {k: np.asarray(v) for k, v in load_pkg("synth").seeded_state_dict(seed, norm="batch").items()}


def bn_net(gx=GX, gy=GY, seed=0, max_batch=4):
    cfg = small_cfg(gx, gy, max_batch)
    load_pkg("framework.voxel_generator").VoxelGenerator(cfg)
    net = load_pkg("networks.pointpillars8_export").PointPillars(cfg)
    net.load_state_dict(bn_sd(seed))
    return net, cfg


# ------------------------------------------------------------------ 1. the fold and the affine gradient
def test_fold_and_affine_grad():
    eng = engine()
    rng = np.random.default_rng(1)
    for C in (64, 128, 256):
        bn = norm_params(rng, C)
        scale, shift = eng.bn_fold(*[dev(t) for t in bn])
        want = R.fold32(*bn)
        assert np.array_equal(scale.cpu().numpy(), want[0]) and np.array_equal(shift.cpu().numpy(), want[1]), C  # each value rounded once
        ds, dh = rng.standard_normal(C) * 50, rng.standard_normal(C) * 50
        ds = bn[2] * dh + ds * 1e-3  # dscale - running_mean dshift cancels to a thousandth
        dg, db = eng.bn_affine_grad(dev(ds), dev(dh), dev(bn[2]), dev(bn[3]))
        rg, rb = R.affine_grad(ds, dh, bn[2], bn[3])
        r = 1.0 / np.sqrt(bn[3].astype(np.float64) + 1e-3)
        check_bound(dg, rg, R.U32 * np.abs(rg) + 8 * R.U64 * r * (np.abs(ds) + np.abs(bn[2] * dh)) + 1e-45, f"dgamma {C}")
        assert np.array_equal(db.cpu().numpy(), dh.astype(np.float32))
    with pytest.raises(ValueError):
        eng.bn_fold(*[dev(t) for t in norm_params(rng, 257)])
    with pytest.raises(TypeError):
        eng.bn_fold(*[torch.from_numpy(t) for t in norm_params(rng, 64)])


# ------------------------------------------------------------------ 2. the primitives: tile edges, halos, K ranges, frames
def unit_case(C, h, w, nb, seed):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((nb, C, h, w)).astype(np.float32)
    wt = (rng.standard_normal((C, C, 3, 3)) * 0.05).astype(np.float32)
    dz, dskip = rng.standard_normal((nb, C, h, w)).astype(np.float32), rng.standard_normal((nb, C, h, w)).astype(np.float32)
    return u, wt, R.fold32(*norm_params(rng, C)), dz, dskip


@pytest.mark.parametrize("C,h,w,nb,norm", [(64, 33, 17, 2, "instance"), (128, 8, 6, 2, "instance"), (256, 3, 2, 3, "instance"),
                                           (128, 8, 6, 2, "batch")])  # a context of either norm kind takes the call
def test_unit(C, h, w, nb, norm):
    load_pkg().install()
    eng = engine() if norm == "instance" else ENG(small_cfg(24, 16, 3), norm="batch")
    u, wt, (sc, sh), dz, dskip = unit_case(C, h, w, nb, 200 + C + h)
    ud, wd, scd, shd, dzd, dsd = (dev(t) for t in (u, wt, sc, sh, dz, dskip))
    got = eng.unit_backward_affine(ud, wd, scd, shd, dzd)
    want, bounds = R.unit_bounds(u, wt, sc, sh, dz)
    check_all(got, want, bounds, f"unit {C}x{h}x{w}x{nb}")
    assert same(got, eng.unit_backward_affine(ud, wd, scd, shd, dzd))  # two runs
    dw3, du3, ds3, dh3 = eng.unit_backward_affine(ud, wd, scd, shd, dzd, need_affine=False)
    assert ds3 is None and dh3 is None and torch.equal(dw3, got[0]) and torch.equal(du3, got[1])
    dw4, none, _, _ = eng.unit_backward_affine(ud, wd, scd, shd, dzd, need_du=False, need_affine=False)
    assert none is None and torch.equal(dw4, got[0])
    skip = eng.unit_backward_affine(ud, wd, scd, shd, dzd, dskip=dsd)
    assert torch.equal(skip[0], got[0]) and torch.equal(skip[1], got[1] + dsd) and same(skip[2:], got[2:])  # dskip is exactly one fp32 add
    want, bounds = R.unit_bounds(u, wt, sc, sh, dz, dskip=dskip)
    check_all(skip, want, bounds, f"unit {C}x{h}x{w}x{nb} + dskip")
    for f in range(nb):  # a frame's du does not depend on the batch it rides in
        s = slice(f, f + 1)
        one = eng.unit_backward_affine(dev(u[s]), wd, scd, shd, dev(dz[s]), dskip=dev(dskip[s]))
        assert torch.equal(one[1][0], skip[1][f]), f


def down_case(cin, cout, hin, win, nb, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nb, cin, hin, win)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3)) * 0.05).astype(np.float32)
    z = R.D.conv_s2(x, wt).astype(np.float32)
    dy = rng.standard_normal(z.shape).astype(np.float32)
    return x, wt, z, R.fold32(*norm_params(rng, cout)), dy


@pytest.mark.parametrize("cin,cout,hin,win", [(64, 64, 32, 24), (64, 128, 17, 9), (128, 256, 8, 6)])
def test_down(cin, cout, hin, win):
    eng = engine()
    nb = 2
    x, wt, z, (sc, sh), dy = down_case(cin, cout, hin, win, nb, 300 + cout + hin)
    xd, wd, zd, scd, shd, dyd = (dev(t) for t in (x, wt, z, sc, sh, dy))
    got = eng.down_backward_affine(xd, wd, zd, scd, shd, dyd)
    want, bounds = R.down_bounds(x, wt, z, sc, sh, dy)
    check_all(got, want, bounds, f"down {cin}->{cout} {hin}x{win}")
    assert same(got, eng.down_backward_affine(xd, wd, zd, scd, shd, dyd))
    dw3, none, ds3, dh3 = eng.down_backward_affine(xd, wd, zd, scd, shd, dyd, need_dx=False)
    assert none is None and torch.equal(dw3, got[0]) and torch.equal(ds3, got[2]) and torch.equal(dh3, got[3])
    assert eng.down_backward_affine(xd, wd, zd, scd, shd, dyd, need_affine=False)[2:] == (None, None)
    for f in range(nb):
        s = slice(f, f + 1)
        assert torch.equal(eng.down_backward_affine(dev(x[s]), wd, dev(z[s]), scd, shd, dev(dy[s]))[1][0], got[1][f]), f


@pytest.mark.parametrize("branch", [0, 1, 2])
def test_neck(branch):
    eng = engine()  # 24 x 16 cells: H, W = 12, 8
    nb = 2
    rng = np.random.default_rng(400 + branch)
    (cin, h, w), wsh = eng.neck_shapes(branch)
    cup, coff = wsh[1], R.N.COFF[branch]
    x = rng.standard_normal((nb, cin, h, w)).astype(np.float32)
    wt = (rng.standard_normal(wsh) * 0.05).astype(np.float32)
    sc, sh = R.fold32(*norm_params(rng, cup))
    y = rng.standard_normal((nb, 320, eng.H, eng.W)).astype(np.float32)  # the mask is the given y, whatever the forward would give
    y[:, coff:coff + cup] = np.maximum(R.aff(R.N.conv_t(x, wt), sc, sh), 0.0).astype(np.float32)
    y[0, coff, 0, :3] = (0.0, 1.0, 0.0)  # and not a recomputed sign
    dy = rng.standard_normal(y.shape).astype(np.float32)
    xd, wd, scd, shd, yd, dyd = (dev(t) for t in (x, wt, sc, sh, y, dy))
    got = eng.neck_backward_affine(branch, xd, wd, scd, shd, yd, dyd)
    sl = slice(coff, coff + cup)
    want, bounds = R.branch_backward(x, wt, sc, y[:, sl], dy[:, sl], bounds=True)
    check_all(got, want, bounds, f"neck {branch}")
    assert same(got, eng.neck_backward_affine(branch, xd, wd, scd, shd, yd, dyd))
    dw3, none, ds3, dh3 = eng.neck_backward_affine(branch, xd, wd, scd, shd, yd, dyd, need_dx=False)
    assert none is None and torch.equal(dw3, got[0]) and torch.equal(ds3, got[2]) and torch.equal(dh3, got[3])
    for f in range(nb):
        s = slice(f, f + 1)
        assert torch.equal(eng.neck_backward_affine(branch, dev(x[s]), wd, scd, shd, dev(y[s]), dev(dy[s]))[1][0], got[1][f]), f


def test_bad_arguments_raise_and_the_next_call_works():
    eng = engine()
    u, wt, (sc, sh), dz, _ = unit_case(64, 5, 4, 2, 9)
    ud, wd, scd, shd, dzd = (dev(t) for t in (u, wt, sc, sh, dz))
    base = eng.unit_backward_affine(ud, wd, scd, shd, dzd)
    with pytest.raises(ValueError):
        eng.unit_backward_affine(ud, wd, scd, shd, dzd, need_du=False)  # the sums need du
    with pytest.raises(ValueError):
        eng.unit_backward_affine(ud, wd, scd[:-1], shd, dzd)
    with pytest.raises(TypeError):
        eng.unit_backward_affine(ud, wd, scd.cpu(), shd, dzd)
    with pytest.raises(ValueError):
        eng.unit_backward_affine(torch.cat([ud] * 2), wd, scd, shd, torch.cat([dzd] * 2))  # nb = 4 > max_batch
    x, wk, z, (s2, h2), dy = down_case(64, 64, 6, 4, 1, 10)
    with pytest.raises(TypeError):
        eng.down_backward_affine(dev(x), dev(wk), dev(z), dev(s2), dev(h2.astype(np.float64)), dev(dy))
    with pytest.raises(ValueError):
        eng.neck_backward_affine(3, ud, wd, scd, shd, ud, ud)
    lib, p = eng.lib, lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dw, du, ds = torch.empty_like(wd), torch.empty_like(ud), torch.empty(64, dtype=torch.float64, device="cuda")
    call = lambda du_, ds_, dh_: lib.pp_unit_backward_affine(eng.ctx, 64, 5, 4, p(ud), p(wd), p(scd), p(shd), p(dzd), None, 2, p(dw),  # noqa: E731
                                                             du_, ds_, dh_, None)
    assert call(None, p(ds), p(ds)) != 0 and b"need du" in lib.pp_last_error(eng.ctx)
    assert call(p(du), p(ds), None) != 0 and b"go together" in lib.pp_last_error(eng.ctx)
    assert call(p(du), ctypes.c_void_p(ds.data_ptr() + 4), p(ds)) != 0 and b"8-byte" in lib.pp_last_error(eng.ctx)
    assert lib.pp_unit_backward_affine(eng.ctx, 64, 5, 4, p(ud), p(wd), None, p(shd), p(dzd), None, 2, p(dw), p(du), None, None, None) != 0
    assert same(eng.unit_backward_affine(ud, wd, scd, shd, dzd), base)
    # the fold's refusals: before the first commit, and on an InstanceNorm context
    sd = bn_sd()
    tensors = {f"{pfx}.{s}": dev(np.asarray(sd[f"{pfx}.{s}"], np.float32)) for pfx, _ in ENG.bn_layers() for s in ENG.BN_FIELDS}
    empty = ENG(small_cfg(24, 16, 2), norm="batch")
    with pytest.raises(RuntimeError, match="not committed"):
        empty.update_bn_fold(tensors)
    with pytest.raises(RuntimeError, match="BatchNorm backbone only"):
        _instance_engine().update_bn_fold(tensors)
    with pytest.raises(KeyError):
        empty.update_bn_fold({k: v for k, v in tensors.items() if k != "rpn.deconv3.1.bias"})


def _instance_engine():
    eng = ENG(small_cfg(24, 16, 2))
    eng.load_state_dict({k: np.asarray(v, np.float32) for k, v in load_pkg("synth").seeded_state_dict(0).items()})
    return eng


# ------------------------------------------------------------------ 3. the fold in place, through every pass
TX, TY = 128, 160  # cells: the level-0 map is 64 x 80 = 4 x 5 tiles of 16 x 16, the geometry of test_tile_skip_gpu.py


def test_update_bn_fold_reaches_every_pass(monkeypatch):
    """backbone(), pp_infer_frame and pp_infer_batch (sparse first convolution, tile skipping at level 0 where the plan runs it) after
    an in-place fold of perturbed tensors, against a fresh engine that loaded the same state_dict: nothing derived from the affine
    survives from the pass before."""
    monkeypatch.setenv("PP_FORCE_VARIANT", "wino6;k3s2 tw16 w1x4 t4x5 bx1 kc4")
    load_pkg().install()

    def make(sd):
        cfg = small_cfg(TX, TY, 2)
        cfg["max_voxels"] = 4000
        eng = ENG(cfg, norm="batch")
        eng.load_state_dict(sd)
        eng.set_sparse_conv1(True)
        eng.set_tile_skip(True)
        return eng

    rng = np.random.default_rng(9)
    pts = [dev(rng.uniform([8.0, 10.0, -1.5, 0], [14.0, 17.0, 1.0, 1], (4000, 4)).astype(np.float32)) for _ in range(2)]

    def passes(eng):
        v, c, n, num = eng.voxelize(pts[0])
        k = int(num.item())
        feat = eng.pfn(v[:k].contiguous(), c[:k].contiguous(), n[:k].contiguous(), eng.num_tensor(k))
        out = [eng.backbone(eng.scatter(feat, c[:k].contiguous(), eng.num_tensor(k))).clone()]
        det, cnt = eng.infer_frame(pts[0])
        torch.cuda.synchronize()
        assert int(eng.fetch(0, "active")[0]) > 0  # the sparse first convolution ran
        skipped = eng.tile_skip_active()
        out += [eng.fetch(0, "rpn").clone(), det.clone(), cnt.clone()]
        det, cnt = eng.infer_batch(pts)
        torch.cuda.synchronize()
        out += [eng.fetch(1, "rpn").clone(), det.clone(), cnt.clone()]
        return out, skipped

    sd = bn_sd()
    eng = make(sd)
    base, skipped = passes(eng)
    assert skipped  # the BatchNorm plan runs tile skipping on this geometry: relu(shift) is the constant outside the active set
    new = dict(sd)
    for pfx, c in ENG.bn_layers():
        g, b, rm, rv = norm_params(rng, c)
        new.update({pfx + ".weight": sd[pfx + ".weight"] * g, pfx + ".bias": sd[pfx + ".bias"] + b, pfx + ".running_mean": sd[pfx + ".running_mean"] + rm,
                    pfx + ".running_var": sd[pfx + ".running_var"] * rv})
    tensors = lambda d: {f"{pfx}.{s}": dev(np.asarray(d[f"{pfx}.{s}"], np.float32)) for pfx, _ in ENG.bn_layers() for s in ENG.BN_FIELDS}  # noqa: E731
    fresh = make(new)
    assert fresh.layer_tilings() == eng.layer_tilings()
    want, skipped2 = passes(fresh)
    assert skipped2 == skipped and (want[0] - base[0]).abs().max() > 1e-3
    for which, d, ref in (("new", new, want), ("old", sd, base), ("new", new, want)):
        eng.update_bn_fold(tensors(d))
        got, _ = passes(eng)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(a, b), (which, i)


# ------------------------------------------------------------------ 4. the autograd surface
def stacked_taps(eng, canvases):
    outs = [eng.backbone_train_taps(c) for c in canvases]
    y = torch.cat([o[0] for o in outs])
    units = [[torch.stack([o[2][b][k] for o in outs]) for k in range(ENG.RPN_UNITS[b])] for b in range(3)]
    return y, units, [torch.cat([o[3][b] for o in outs]) for b in range(3)]


def test_fixture_chain():
    """The fixture's tensors through the network against the reference's float64 gradients; the ReLU masks are compared first."""
    load_pkg().install()
    shared = load_pkg("networks.pointpillars8_shared")
    g = golden("bntrain_small")
    canvas, ws, bn, dy = small_inputs()
    wc, wn = split(ws)
    net, _ = bn_net(canvas.shape[2], canvas.shape[3], max_batch=2)
    sd = bn_sd()
    for k, w in zip(R.LAYER_KEYS, ws):
        assert sd[k].shape == w.shape, k
        sd[k] = w
    for pfx, t in zip(R.BN_PREFIXES, bn):
        sd.update({f"{pfx}.{s}": v for s, v in zip(ENG.BN_FIELDS, t)})
    net.load_state_dict(sd)
    eng = net._eng
    cv = dev(canvas)
    fwd = R.rpn_forward(canvas, wc, wn, dict(zip(R.BN_PREFIXES, bn)))
    y, units, zs = stacked_taps(eng, cv)
    want = R.relu_masks(fwd["y"], fwd["units"], fwd["zs"], fwd["folds"])
    folds32 = {p: R.fold32(*t) for p, t in zip(R.BN_PREFIXES, bn)}
    got = R.relu_masks(y.cpu().numpy(), [[u.cpu().numpy() for u in us] for us in units], [z.cpu().numpy() for z in zs], folds32)
    for site in want:
        flipped = int((want[site] != got[site]).sum())
        assert flipped == 0, f"ReLU mask flipped at {site}: {flipped} of {want[site].size} elements take another branch on the GPU than in float64"
    net.train(scope="rpn", bn_stats="frozen")
    names = [k for k, _ in net.named_parameters()]
    assert names == [str(k) for k in g["param_names"]] + list(shared.HEAD_KEYS) and len(names) == 63
    cvg = cv.clone().requires_grad_()
    out = net.rpn_train(cvg)
    assert torch.equal(out.detach(), torch.cat([net.rpn(c) for c in cv])) and torch.equal(out.detach(), y)  # the inference bits
    # frozen statistics do not normalise this input: rpn_out runs into the hundreds, and the bar scales with it
    assert np.abs(out.detach().cpu().numpy() - fwd["y"]).max() <= BAR * max(1.0, np.abs(fwd["y"]).max())
    out.backward(dev(dy))
    params = dict(net.named_parameters())
    for i, k in enumerate(names[:57]):
        got = params[k].grad.reshape(-1)
        check_grad(got[::DW_STRIDE] if params[k].dim() == 4 else got, g[f"g_{i}"], float(g[f"ref32_dev_g_{i}"]), float(g[f"g_{i}_max"]), f"golden {k}")
    check_grad(cvg.grad.reshape(-1)[::DX_STRIDE], g["dcanvas"], float(g["ref32_dev_dcanvas"]), float(g["dcanvas_max"]), "golden dcanvas")


def test_scopes():
    """Every scope returns the inference bits and, for the tensors it shares with "rpn", the same gradient bits; "neck" leaves
    everything in front untouched and asks for no dx; "all" composes with the PFN backward."""
    load_pkg().install()
    shared = load_pkg("networks.pointpillars8_shared")
    net, _ = bn_net()
    eng = net._eng
    example = two_frames(eng)
    plain = net(example)
    assert all(v.grad_fn is None for v in plain.values())
    rng = np.random.default_rng(8)
    up = {k: dev(rng.standard_normal(tuple(v.shape)).astype(np.float32) * np.float32(1e-2)) for k, v in plain.items()}
    grads = {}
    for scope in ("neck", "block3", "stage3", "rpn"):
        net.train(scope=scope, bn_stats="frozen")
        preds = net(example)
        for k in plain:
            assert preds[k].requires_grad and torch.equal(preds[k].detach(), plain[k]), (scope, k)
        net.zero_grad()
        sum((preds[k] * up[k]).sum() for k in preds).backward()
        grads[scope] = {k: p.grad.clone() for k, p in net.named_parameters()}
        assert all(float(v.abs().max()) > 0 for v in grads[scope].values()), scope
    assert [len(grads[s]) for s in ("neck", "block3", "stage3", "rpn")] == [15, 30, 33, 63]
    for scope in ("neck", "block3", "stage3"):
        for k, v in grads[scope].items():
            assert torch.equal(v, grads["rpn"][k]), (scope, k)
    # "neck": the three upsamplers with their norms, by hand, without dx
    net.train(scope="neck", bn_stats="frozen")
    frames = canvases_of(eng, example)
    calls = []
    real = eng.neck_backward  # the walk hands the frozen norm over as a record: norm=BackwardNorm(scale, shift, need_affine=...)
    eng.neck_backward = lambda *a, **kw: calls.append({**kw, "need_affine": kw["norm"].mean is None and kw["norm"].need_affine}) or real(*a, **kw)
    try:
        y = net.rpn_train(torch.cat(frames))
        gh, dxh = eng.head_backward(y.detach(), up["cls_preds"], up["box_preds"], up["dir_preds"])
        net.zero_grad()
        y.backward(dxh)
    finally:
        del eng.neck_backward
    assert len(calls) == 3 and not any(kw["need_dx"] for kw in calls) and all(kw["need_affine"] for kw in calls)
    taps = [eng.backbone_taps(c) for c in frames]
    p = {k: v.detach() for d in (net._neck, net._bn_run) for k, v in d.items()}
    for b, key in enumerate(shared.NECK_KEYS):
        pfx = ENG.bn_prefix(key)
        sc, sh = eng.bn_fold(*[p[f"{pfx}.{s}"] for s in ENG.BN_FIELDS])
        dw, none, ds, dh = eng.neck_backward_affine(b, torch.cat([t[1 + b] for t in taps]), p[key], sc, sh, y.detach(), dxh, need_dx=False)
        dg, db = eng.bn_affine_grad(ds, dh, p[pfx + ".running_mean"], p[pfx + ".running_var"])
        assert none is None
        for k, v in ((key, dw), (pfx + ".weight", dg), (pfx + ".bias", db)):
            assert torch.equal(net._neck[k].grad, v) and torch.equal(v, grads["rpn"][k]), k
    assert all(q.grad is None for d in (net._rpn, net._down, net._block) for q in d.values())
    # "all": the canvases' gradient reaches the pillar feature net
    net.train(scope="all", bn_stats="frozen")
    names = [k for k, _ in net.named_parameters()]
    assert names == list(shared.BN_ALL_KEYS) and len(names) == 66
    rm0 = net._pfn_stats[shared.PFN_STAT_KEYS[0]].clone()
    preds = net(example)
    net.zero_grad()
    sum((preds[k] * up[k]).sum() for k in preds).backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() and float(q.grad.abs().max()) > 0 for q in net.parameters())
    assert not torch.equal(net._pfn_stats[shared.PFN_STAT_KEYS[0]], rm0)  # the PFN's BatchNorm1d runs in train mode, as on the InstanceNorm network
    net.eval()
    assert [k for k, _ in net.named_parameters()] == list(shared.HEAD_KEYS)


def test_trajectory():
    """Twenty Adam steps of the reference's loop body (forward, LossGenerator.generate, backward, clip, Adam) on a fixed batch of two
    frames under train(scope="all", bn_stats="frozen"): the loss falls, all 66 tensors move, the running statistics of the RPN do not,
    and a fresh network loaded with state_dict() computes the same bits through every pass."""
    load_pkg().install()
    shared = load_pkg("networks.pointpillars8_shared")
    OPT = load_pkg("framework.optim")
    from test_optim_gpu import fixed_batch
    net, cfg = bn_net()
    eng = net._eng
    example, ex = two_frames(eng), fixed_batch(eng)
    lg = load_pkg("framework.loss_generator").LossGenerator(cfg)
    net.load_state_dict({**bn_sd(), **{pfx + ".num_batches_tracked": np.asarray(7, np.int64) for pfx, _ in ENG.bn_layers()}})
    start = net.state_dict()
    net.train(scope="all", bn_stats="frozen")
    opt = OPT.Adam(net.parameters(), lr=1e-3)
    losses = []
    for _ in range(20):
        loss = lg.generate(net(example), ex)["loss"]
        opt.zero_grad()
        loss.backward()
        OPT.clip_grad_norm_(net.parameters(), 10.0)
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(lg.generate(net(example), ex)["loss"]))
    print("all, frozen statistics:", " ".join(f"{v:.6f}" for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    net.eval()
    sd = net.state_dict()
    for k in shared.BN_ALL_KEYS:
        assert np.abs(sd[k] - np.asarray(start[k], np.float32).reshape(sd[k].shape)).max() > 0, k  # all 66 moved
    for pfx, _ in ENG.bn_layers():
        for s in ("running_mean", "running_var", "num_batches_tracked"):
            assert np.array_equal(sd[f"{pfx}.{s}"], start[f"{pfx}.{s}"]), (pfx, s)
    other, _ = bn_net()
    other.load_state_dict(sd)
    canvas = canvases_of(eng, example)[0]
    assert torch.equal(other.rpn(canvas), net.rpn(canvas))
    pa, pb = net(example), other(example)
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    rng = np.random.default_rng(5)
    pts = dev(rng.uniform([0, 0, -1.5, 0], [0.2 * GX, 0.2 * GY, 1.0, 1], (3000, 4)).astype(np.float32))
    da, db = eng.infer_frame(pts), other._eng.infer_frame(pts)
    assert torch.equal(eng.fetch(0, "rpn"), other._eng.fetch(0, "rpn")) and all(torch.equal(x, y) for x, y in zip(da, db))


def test_argument_rules():
    load_pkg().install()
    net, _ = bn_net(16, 16, max_batch=2)
    with pytest.raises(RuntimeError, match="InstanceNorm.*bn_stats='frozen'"):
        net.train(scope="rpn")
    with pytest.raises(NotImplementedError):
        net.train(scope="rpn", bn_stats="batch")
    with pytest.raises(ValueError, match="fp32"):
        net.train(scope="rpn", bn_stats="frozen", grad_precision="bf16x3")
    cfg = small_cfg(16, 16, 2)
    load_pkg("framework.voxel_generator").VoxelGenerator(cfg)
    with pytest.raises(ValueError, match="BatchNorm"):
        load_pkg("networks.pointpillars8_shared").PointPillars(cfg).train(scope="rpn", bn_stats="frozen")
    net.train(scope="rpn", bn_stats="frozen")
    cv = torch.zeros((1, 64, 16, 16), dtype=torch.float32, device="cuda")
    good = net.rpn_train(cv)
    net.half()
    with pytest.raises(RuntimeError, match="fp32"):
        net.rpn_train(cv)  # the 16-bit modes raise as on the InstanceNorm network
    net.float()
    again = net.rpn_train(cv)
    assert again.requires_grad and torch.equal(again.detach(), good.detach())
