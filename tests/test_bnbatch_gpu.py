"""GPU: training the BatchNorm network with batch statistics -- the three backward primitives with pooled statistics
(pp_unit_backward_bn, pp_down_backward_bn, pp_neck_backward_bn), the lock-step training forward (pp_backbone_train_taps_bn) and the
autograd surface PointPillars.train(scope=..., bn_stats="moving") of networks.pointpillars8_export -- against the float64 restatement
(tests/bnbatch_ref.py) and the reference's float64 goldens (tests/golden/make_bnbatch_goldens.py).

Bars.  Primitives: the element-wise a-priori bounds of bnbatch_ref (float32 summation in any order from the same float32 inputs; the
mask is exact, no near-ties).  Forward: the project's backbone bar 2e-4 on rpn_out, 2e-4 x max |value| on the statistics.  Fixture
gradients: 4 x ref32_dev x max |g64| per tensor, the bar of test_rpntrain_gpu.py / test_bntrain_gpu.py.  Equality is asserted between
identical calls, with and without du / dx, for the dskip add, across chunk_frames (du / dx and the sums), between scopes, and between
a stepped network and a fresh one that loaded its state_dict()."""
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden, load_pkg
import bnbatch_ref as R
from train_common import GX, GY, canvases_of, check_bound, check_grad, dev, engine, small_cfg, two_frames
from test_bntrain_gpu import ENG, bn_net, bn_sd, check_all, norm_params, same

sys.path.insert(0, GOLDEN)
from make_bnbatch_goldens import DW_STRIDE, DX_STRIDE, Y_STRIDE, small_inputs, split  # noqa: E402

pytestmark = pytest.mark.gpu
BAR = 2e-4  # the project's backbone bar


def folded32(v, rng, C):
    """The batch statistics of v as the library rounds them and their fold with a drawn (gamma, beta) -> scale, shift, mean, var f32."""
    mean, var = R.stats32(v)
    return (*R.fold32(*norm_params(rng, C)[:2], mean, var), mean, var)


def chunks_agree(call, base, bound_w, what):
    """chunk_frames 1 and 2 against the workspace rule: du / dx and the sums keep their bits, dw stays inside its bound."""
    for k in (1, 2):
        got = call(k)
        assert torch.equal(got[1], base[1]) and torch.equal(got[2], base[2]) and torch.equal(got[3], base[3]), (what, k)
        check_bound(got[0], bound_w[0], bound_w[1], f"{what} dw, chunk_frames {k}")


# ------------------------------------------------------------------ 1. the primitives
@pytest.mark.parametrize("C,h,w,nb,norm", [(64, 33, 17, 2, "instance"), (128, 8, 6, 3, "instance"), (256, 3, 2, 3, "instance"),
                                           (128, 8, 6, 3, "batch")])  # a context of either norm kind takes the call
def test_unit(C, h, w, nb, norm):
    load_pkg().install()
    eng = engine() if norm == "instance" else ENG(small_cfg(24, 16, 3), norm="batch")
    rng = np.random.default_rng(500 + C + h)
    u = rng.standard_normal((nb, C, h, w)).astype(np.float32)
    wt = (rng.standard_normal((C, C, 3, 3)) * 0.05).astype(np.float32)
    dz, dskip = rng.standard_normal((nb, C, h, w)).astype(np.float32), rng.standard_normal((nb, C, h, w)).astype(np.float32)
    st = folded32(u, rng, C)
    ud, wd, dzd, dsd = (dev(t) for t in (u, wt, dz, dskip))
    std = [dev(t) for t in st]
    got = eng.unit_backward_bn(ud, wd, *std, dzd)
    want, bounds = R.unit_bounds(u, wt, *st, dz)
    check_all(got, want, bounds, f"unit {C}x{h}x{w}x{nb}")
    assert same(got, eng.unit_backward_bn(ud, wd, *std, dzd))  # two runs
    dw3, du3, ds3, dh3 = eng.unit_backward_bn(ud, wd, *std, dzd, need_affine=False)
    assert ds3 is None and dh3 is None and torch.equal(dw3, got[0]) and torch.equal(du3, got[1])
    dw4, none, _, _ = eng.unit_backward_bn(ud, wd, *std, dzd, need_du=False, need_affine=False)
    assert none is None and torch.equal(dw4, got[0])
    with pytest.raises(ValueError):
        eng.unit_backward_bn(ud, wd, *std, dzd, need_du=False)  # the sums need du
    skip = eng.unit_backward_bn(ud, wd, *std, dzd, dskip=dsd)
    assert torch.equal(skip[0], got[0]) and torch.equal(skip[1], got[1] + dsd) and same(skip[2:], got[2:])  # dskip is exactly one fp32 add
    want, bounds = R.unit_bounds(u, wt, *st, dz, dskip=dskip)
    check_all(skip, want, bounds, f"unit {C}x{h}x{w}x{nb} + dskip")
    if nb == 3:
        chunks_agree(lambda k: eng.unit_backward_bn(ud, wd, *std, dzd, dskip=dsd, chunk_frames=k), skip, (want[0], bounds[0]), f"unit {C}")
    with pytest.raises(ValueError):
        eng.unit_backward_bn(ud, wd, *std, dzd, chunk_frames=-1)
    with pytest.raises(ValueError):
        eng.unit_backward_bn(ud, wd, std[0], std[1], std[2][:-1], std[3], dzd)


@pytest.mark.parametrize("cin,cout,hin,win", [(64, 64, 32, 24), (64, 128, 17, 9), (128, 256, 8, 6)])
def test_down(cin, cout, hin, win):
    eng = engine()
    nb = 3
    rng = np.random.default_rng(600 + cout + hin)
    x = rng.standard_normal((nb, cin, hin, win)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3)) * 0.05).astype(np.float32)
    z = R.D.conv_s2(x, wt).astype(np.float32)
    dy = rng.standard_normal(z.shape).astype(np.float32)
    st = folded32(z, rng, cout)
    xd, wd, zd, dyd = (dev(t) for t in (x, wt, z, dy))
    std = [dev(t) for t in st]
    got = eng.down_backward_bn(xd, wd, zd, *std, dyd)
    want, bounds = R.down_bounds(x, wt, z, *st, dy)
    check_all(got, want, bounds, f"down {cin}->{cout} {hin}x{win}")
    assert same(got, eng.down_backward_bn(xd, wd, zd, *std, dyd))
    dw3, none, ds3, dh3 = eng.down_backward_bn(xd, wd, zd, *std, dyd, need_dx=False)
    assert none is None and torch.equal(dw3, got[0]) and torch.equal(ds3, got[2]) and torch.equal(dh3, got[3])
    assert eng.down_backward_bn(xd, wd, zd, *std, dyd, need_affine=False)[2:] == (None, None)
    chunks_agree(lambda k: eng.down_backward_bn(xd, wd, zd, *std, dyd, chunk_frames=k), got, (want[0], bounds[0]), f"down {cout}")


@pytest.mark.parametrize("branch", [0, 1, 2])
def test_neck(branch):
    eng = engine()  # 24 x 16 cells: H, W = 12, 8
    rng = np.random.default_rng(700 + branch)
    (cin, h, w), wsh = eng.neck_shapes(branch)
    cup, coff = wsh[1], R.N.COFF[branch]
    sl = slice(coff, coff + cup)
    wt = (rng.standard_normal(wsh) * 0.05).astype(np.float32)
    wd = dev(wt)

    def case(nb):
        x = rng.standard_normal((nb, cin, h, w)).astype(np.float32)
        Z = R.N.conv_t(x, wt)
        st = folded32(Z, rng, cup)
        y = rng.standard_normal((nb, 320, eng.H, eng.W)).astype(np.float32)  # the mask is the given y, whatever the forward would give
        y[:, sl] = np.maximum(R.aff(Z, st[0], st[1]), 0.0).astype(np.float32)
        y[0, coff, 0, :3] = (0.0, 1.0, 0.0)  # and not a recomputed sign
        dy = rng.standard_normal(y.shape).astype(np.float32)
        return x, st, y, dy

    x, st, y, dy = case(2)
    xd, yd, dyd = dev(x), dev(y), dev(dy)
    std = [dev(t) for t in st]
    got = eng.neck_backward_bn(branch, xd, wd, *std, yd, dyd)
    want, bounds = R.branch_backward(x, wt, st[0], st[2], st[3], y[:, sl], dy[:, sl], bounds=True)
    check_all(got, want, bounds, f"neck {branch}")
    assert same(got, eng.neck_backward_bn(branch, xd, wd, *std, yd, dyd))
    dw3, none, ds3, dh3 = eng.neck_backward_bn(branch, xd, wd, *std, yd, dyd, need_dx=False)
    assert none is None and torch.equal(dw3, got[0]) and torch.equal(ds3, got[2]) and torch.equal(dh3, got[3])
    x, st, y, dy = case(3)  # several chunks: Z is recomputed for the second round
    xd, yd, dyd = dev(x), dev(y), dev(dy)
    std = [dev(t) for t in st]
    base = eng.neck_backward_bn(branch, xd, wd, *std, yd, dyd)
    want, bounds = R.branch_backward(x, wt, st[0], st[2], st[3], y[:, sl], dy[:, sl], bounds=True)
    check_all(base, want, bounds, f"neck {branch}, three frames")
    chunks_agree(lambda k: eng.neck_backward_bn(branch, xd, wd, *std, yd, dyd, chunk_frames=k), base, (want[0], bounds[0]), f"neck {branch}")


# ------------------------------------------------------------------ 2. the lock-step forward against the fixture
def fixture_net(max_batch=2):
    """The BatchNorm network on the fixture's geometry holding the fixture's weights and norms (num_batches_tracked = 7)."""
    canvas, ws, bn, dy = small_inputs()
    net, _ = bn_net(canvas.shape[2], canvas.shape[3], max_batch=max_batch)
    sd = bn_sd()
    for k, w in zip(R.LAYER_KEYS, ws):
        assert sd[k].shape == w.shape, k
        sd[k] = w
    for pfx, t in zip(R.BN_PREFIXES, bn):
        sd.update({f"{pfx}.{s}": v for s, v in zip(ENG.BN_FIELDS, t)})
        sd[pfx + ".num_batches_tracked"] = np.asarray(7, np.int64)
    net.load_state_dict(sd)
    return net, sd, canvas, ws, bn, dy


@pytest.fixture(scope="module")
def fixture_fwd():
    canvas, ws, bn, _ = small_inputs()
    wc, wn = split(ws)
    return R.rpn_forward(canvas, wc, wn, dict(zip(R.BN_PREFIXES, bn)))


def bn_params(net):
    return {k: p for attr in ("_neck", "_rpn", "_block", "_down") for k, p in getattr(net, attr).items()}


def test_forward_against_the_fixture(fixture_fwd):
    load_pkg().install()
    g = golden("bnbatch_small")
    net, sd, canvas, ws, bn, _ = fixture_net()
    eng, cv, fwd = net._eng, dev(canvas), fixture_fwd
    before = torch.cat([eng.backbone(c) for c in cv])
    y, xs, units, zs, mean, var, scale, shift = eng.backbone_train_taps_bn(cv, bn_params(net))
    assert torch.equal(torch.cat([eng.backbone(c) for c in cv]), before)  # the committed fold of the running statistics is untouched
    again = eng.backbone_train_taps_bn(cv, bn_params(net), taps=2)
    assert again[2][:2] == (None, None) and again[3][0] is None and torch.equal(again[2][2], units[2]) and torch.equal(again[3][2], zs[2])
    assert (again[0] - y).abs().max() <= 1e-5  # the statistics are summed with atomics: the last bits may differ between passes
    err = np.abs(y.cpu().numpy().astype(np.float64).reshape(-1)[::Y_STRIDE] - g["rpn_out"]).max()
    full = np.abs(y.cpu().numpy() - fwd["y"]).max()
    print(f"rpn_out: max abs deviation {full:.3e} (at the golden's stride {err:.3e}), the reference's own float32 run {float(g['ref32_abs_rpn_out']):.3e}")
    assert err <= BAR and full <= BAR
    for i, ((pfx, c), t) in enumerate(zip(ENG.bn_layers(), bn)):
        gamma, beta = dev(t[0]), dev(t[1])
        sc, sh = eng.bn_fold(gamma, beta, mean[i, :c].contiguous(), var[i, :c].contiguous())
        assert torch.equal(sc, scale[i, :c]) and torch.equal(sh, shift[i, :c]), pfx  # pp_bn_fold's bits
        for name, got, want in (("mean", mean, g[f"mean_{i}"]), ("var", var, g[f"var_{i}"])):
            d = np.abs(got[i, :c].cpu().numpy().astype(np.float64) - want).max()
            print(f"{pfx} {name}: max deviation {d:.3e}, {d / np.abs(want).max():.3e} of max |value|")
            assert d <= BAR * np.abs(want).max(), (pfx, name)
        assert float(mean[i, c:].abs().max()) == 0.0 if c < 256 else True
    # the taps, and the branch every ReLU takes
    for b in range(3):
        assert units[b].shape[:2] == (ENG.RPN_UNITS[b], 2) and zs[b].shape[0] == 2
        for got, want in [(xs[b], fwd["taps"][b]), (zs[b], fwd["zs"][b])] + [(units[b][k], fwd["units"][b][k]) for k in range(ENG.RPN_UNITS[b])]:
            assert np.abs(got.cpu().numpy() - want).max() <= BAR * max(1.0, np.abs(want).max())
    folds32 = {p: (scale[i, :c].cpu().numpy(), shift[i, :c].cpu().numpy()) for i, (p, c) in enumerate(ENG.bn_layers())}
    want = R.relu_masks(fwd)
    got = R.A.relu_masks(y.cpu().numpy(), [[u.cpu().numpy() for u in us] for us in units], [z.cpu().numpy() for z in zs], folds32)
    for site in want:
        flipped = int((want[site] != got[site]).sum())
        assert flipped == 0, f"ReLU mask flipped at {site}: {flipped} of {want[site].size} elements take another branch on the GPU than in float64"


def test_one_frame_without_affine_is_the_instance_norm_backbone():
    load_pkg().install()
    net, sd, canvas, ws, bn, _ = fixture_net()
    inst = ENG(small_cfg(canvas.shape[2], canvas.shape[3], 2))
    isd = {k: np.asarray(v, np.float32) for k, v in load_pkg("synth").seeded_state_dict(0).items()}
    isd.update({k: sd[k] for k in R.LAYER_KEYS})
    inst.load_state_dict(isd)
    params = bn_params(net)
    for pfx, c in ENG.bn_layers():
        params[pfx + ".weight"], params[pfx + ".bias"] = torch.ones(c, device="cuda"), torch.zeros(c, device="cuda")
    cv = dev(canvas)
    for f in range(2):
        y = net._eng.backbone_train_taps_bn(cv[f:f + 1], params, taps=False)[0]
        want = inst.backbone_train_taps(cv[f:f + 1])[0]
        d = float((y - want).abs().max())
        print(f"frame {f}: max deviation from the InstanceNorm backbone {d:.3e}")
        assert d <= BAR


# ------------------------------------------------------------------ 3. the autograd surface
def test_fixture_chain(fixture_fwd):
    """The fixture's tensors through train(scope="rpn", bn_stats="moving") against the reference's float64 gradients, and the running
    statistics after the one forward."""
    load_pkg().install()
    shared = load_pkg("networks.pointpillars8_shared")
    g = golden("bnbatch_small")
    net, sd, canvas, ws, bn, dy = fixture_net()
    net.train(scope="rpn", bn_stats="moving")
    names = [k for k, _ in net.named_parameters()]
    assert names == [str(k) for k in g["param_names"]] + list(shared.HEAD_KEYS) and len(names) == 63
    cvg = dev(canvas).requires_grad_()
    out = net.rpn_train(cvg)
    assert np.abs(out.detach().cpu().numpy() - fixture_fwd["y"]).max() <= BAR
    out.backward(dev(dy))
    params = dict(net.named_parameters())
    for i, k in enumerate(names[:57]):
        got = params[k].grad.reshape(-1)
        check_grad(got[::DW_STRIDE] if params[k].dim() == 4 else got, g[f"g_{i}"], float(g[f"ref32_dev_g_{i}"]), float(g[f"g_{i}_max"]), f"golden {k}")
    check_grad(cvg.grad.reshape(-1)[::DX_STRIDE], g["dcanvas"], float(g["ref32_dev_dcanvas"]), float(g["dcanvas_max"]), "golden dcanvas")
    after = net.state_dict()
    for i, (pfx, _) in enumerate(ENG.bn_layers()):
        for s, want in (("running_mean", g[f"rm_{i}"]), ("running_var", g[f"rv_{i}"])):
            d = np.abs(after[f"{pfx}.{s}"].astype(np.float64) - want).max()
            assert d <= BAR * np.abs(want).max() and not np.array_equal(after[f"{pfx}.{s}"], sd[f"{pfx}.{s}"]), (pfx, s, d)
        assert int(after[pfx + ".num_batches_tracked"]) == 8, pfx
    # a partial scope walks less far and gives the same bits where it walks; the statistics move under it as well, and without grad
    grads = {k: params[k].grad.clone() for k in names[:57]}
    net.load_state_dict(sd)
    net.train(scope="neck", bn_stats="moving")
    assert len(list(net.parameters())) == 15
    net.rpn_train(dev(canvas)).backward(dev(dy))
    for k in shared.NECK_KEYS:
        for n in (k, *shared.bn_affine_keys(k)):
            assert torch.equal(net._neck[n].grad, grads[n]), n
    assert all(q.grad is None for d in (net._rpn, net._down, net._block) for q in d.values())
    with torch.no_grad():
        y = net.rpn_train(dev(canvas))
    assert not y.requires_grad and int(net.state_dict()["rpn.block1.1.num_batches_tracked"]) == 9
    with pytest.raises(NotImplementedError, match="moving"):
        net.train(scope="rpn", bn_stats="batch")


def test_step_then_eval():
    """One SGD step under train(scope="rpn", bn_stats="moving"), then eval(): all 63 tensors and all 38 running statistics moved, and a
    fresh network that loaded state_dict() computes the same bits -- the moved statistics were folded again and the training pass left
    nothing in the committed fold -- through rpn() and pp_infer_frame."""
    load_pkg().install()
    shared = load_pkg("networks.pointpillars8_shared")
    net, _ = bn_net()
    eng = net._eng
    example = two_frames(eng)
    start = net.state_dict()
    net.train(scope="rpn", bn_stats="moving")
    preds = net(example)
    sum((v * v).mean() for v in preds.values()).backward()
    with torch.no_grad():
        for p in net.parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all()
            p -= 1e-2 * p.grad / (p.grad.abs().max() + 1e-12)
    net.eval()
    sd = net.state_dict()
    for k in shared.BN_RPN_KEYS:
        assert np.abs(sd[k] - np.asarray(start[k], np.float32).reshape(sd[k].shape)).max() > 0, k
    for pfx, _ in ENG.bn_layers():
        for s in ("running_mean", "running_var"):
            assert np.abs(sd[f"{pfx}.{s}"] - start[f"{pfx}.{s}"]).max() > 0, (pfx, s)
    other, _ = bn_net()
    other.load_state_dict(sd)
    canvas = canvases_of(eng, example)[0]
    a, b = net.rpn(canvas), other.rpn(canvas)
    assert torch.equal(a, b)
    pa, pb = net(example), other(example)
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    rng = np.random.default_rng(5)
    pts = dev(rng.uniform([0, 0, -1.5, 0], [0.2 * GX, 0.2 * GY, 1.0, 1], (3000, 4)).astype(np.float32))
    da, db = eng.infer_frame(pts), other._eng.infer_frame(pts)
    assert torch.equal(eng.fetch(0, "rpn"), other._eng.fetch(0, "rpn")) and all(torch.equal(x, y) for x, y in zip(da, db))


def test_scope_all_steps_with_the_pfn_in_front():
    load_pkg().install()
    shared = load_pkg("networks.pointpillars8_shared")
    net, _ = bn_net()
    example = two_frames(net._eng)
    start = net.state_dict()
    net.train(scope="all", bn_stats="moving")
    assert [k for k, _ in net.named_parameters()] == list(shared.BN_ALL_KEYS)
    preds = net(example)
    sum((v * v).mean() for v in preds.values()).backward()
    with torch.no_grad():
        for p in net.parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0
            p -= 1e-2 * p.grad / p.grad.abs().max()
    net.eval()
    sd = net.state_dict()
    moved = [k for k in shared.BN_ALL_KEYS if np.abs(sd[k] - np.asarray(start[k], np.float32).reshape(sd[k].shape)).max() > 0]
    assert len(moved) == 66
    assert not np.array_equal(sd["rpn.deconv3.1.running_var"], start["rpn.deconv3.1.running_var"])
    assert not np.array_equal(sd[shared.PFN_STAT_KEYS[0]], start[shared.PFN_STAT_KEYS[0]])
