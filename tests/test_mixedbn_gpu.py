"""GPU: the mixed-precision BatchNorm backwards (pp_{unit,down,neck}_backward_affine_mp / _bn_mp, csrc/block_train16.hip,
down_train16.hip, neck_train16.hip) through the engine wrappers (norm=..., bn_grad_precision=...) and through the autograd surface
PointPillars.train(scope=..., bn_stats=..., bn_grad_precision=..., grad_stages=...) of networks.pointpillars8_export.

Bars.  Mode 0 is asserted equal, bit for bit, to the fp32 entries.  Modes 1 and 2 are held to the element-wise a-priori bounds of
tests/mixedbn_ref.py (derived there, cleared on the CPU by tests/test_mixedbn_cpu.py for every input set used here); every largest
fraction of a bound is printed.  Equality with the fp32 entry is asserted for what a mode may not touch (the stage's and the branch's
two sums, the unit's mask) and for every output on exact-arithmetic data, which is what catches an indexing error; equality is asserted
between identical calls, with and without du / dx, for the dskip add, for a frame whatever batch it rides in (affine form), across
chunk_frames (batch form: du / dx and the sums), and between bn_grad_precision="fp32" and a run without the keyword.

Final losses of test_it_trains measured on an MI355X: see DESIGN.md section 4, "Mixed-precision training of the BatchNorm networks"."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import load_pkg
import bntrain_ref as RA
import mixedbn_ref as R
import mixedstage_ref as S
from train_common import check_bound, dev, small_cfg, two_frames
from test_bnbatch_gpu import fixture_net
from test_bntrain_gpu import bn_net, same

pytestmark = pytest.mark.gpu
MODES = ("bf16x3", "bf16")
NETWORK_UNITS = [(64, 400, 400), (128, 200, 200), (256, 100, 100)]
NETWORK_DOWNS = [(64, 64, 800, 800), (64, 128, 400, 400), (128, 256, 200, 200)]
_ENGINES = {}


def engine(gx=24, gy=16, max_batch=3, norm="instance"):
    """An engine without weights (the backwards are stateless and take a context of either norm kind), one per geometry."""
    key = (gx, gy, max_batch, norm)
    if key not in _ENGINES:
        load_pkg().install()
        _ENGINES[key] = load_pkg("engine").Engine(small_cfg(gx, gy, max_batch), norm=norm)
    return _ENGINES[key]


def bnorm(normd, **kw):
    return load_pkg("engine").BackwardNorm(*normd, **kw)


def unit(eng, ud, wd, normd, dzd, prec="fp32", dskip=None, need_du=True, need_affine=True, chunk_frames=0):
    extra = {"chunk_frames": chunk_frames} if len(normd) == 4 else {}
    return eng.unit_backward(ud, wd, dzd, dskip=dskip, need_du=need_du, norm=bnorm(normd, need_affine=need_affine, **extra), bn_grad_precision=prec)


def down(eng, xd, wd, zd, normd, dyd, prec="fp32", need_dx=True, chunk_frames=0):
    extra = {"chunk_frames": chunk_frames} if len(normd) == 4 else {}
    return eng.down_backward(xd, wd, zd, dyd, need_dx=need_dx, norm=bnorm(normd, **extra), bn_grad_precision=prec)


def neck(eng, b, xd, wd, normd, yd, dyd, prec="fp32", need_dx=True, chunk_frames=0):
    extra = {"chunk_frames": chunk_frames} if len(normd) == 4 else {}
    return eng.neck_backward(b, xd, wd, yd, dyd, need_dx=need_dx, norm=bnorm(normd, **extra), bn_grad_precision=prec)


def check(got, want, bounds, what, names=("dw", "dx", "dscale", "dshift")):
    for name, g, w, b in zip(names, got, want, bounds):
        assert g.dtype == (torch.float64 if name[1] == "s" else torch.float32), name
        frac, worst = R.worst(g.cpu().numpy(), w, b)
        print(f"{what} {name}: largest fraction of the a-priori bound {frac:.3f} (largest deviation {worst:.3e})")
        assert frac <= 1.0, (what, name, frac)


def devs(ts):
    return [dev(t) for t in ts]


@functools.lru_cache(maxsize=None)
def unit_set(shape, form):
    """The case, its tensors on the device and the mode-independent terms of its bounds: computed once, shared by both modes."""
    u, w, norm, dz, dskip = R.unit_case(*shape, form)
    return (u, w, norm, dz, dskip), (dev(u), dev(w), devs(norm), dev(dz), dev(dskip)), R.unit_terms(u, w, norm, dz)


@functools.lru_cache(maxsize=None)
def down_set(shape, form):
    x, w, z, norm, dy = R.down_case(*shape, form)
    return (x, w, z, norm, dy), (dev(x), dev(w), dev(z), devs(norm), dev(dy)), R.down_terms(x, w, z, norm, dy)


@functools.lru_cache(maxsize=None)
def neck_set(shape, form):
    xs, ws, norms, y, dy = R.neck_case(*shape, form)
    terms = [R.neck_terms(xs[b], ws[b], norms[b], y[:, S.branch_slice(b)], dy[:, S.branch_slice(b)]) for b in range(3)]
    return (xs, ws, norms, y, dy), (devs(xs), devs(ws), [devs(n) for n in norms], dev(y), dev(dy)), terms


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def c_entry(eng, fam, mode, ints, pre, normd, post, nb, shapes, chunk_frames=0):
    """The C entry pp_<fam>_backward_{affine,bn}_mp itself on fresh outputs -> (dw, dx, dscale, dshift), rc."""
    form = "bn" if len(normd) == 4 else "affine"
    C = normd[1].shape[0]
    outs = [torch.full(s, float("nan"), device="cuda") for s in shapes] + [torch.full((C,), float("nan"), device="cuda", dtype=torch.float64) for _ in range(2)]
    tail = [chunk_frames] if form == "bn" else []
    rc = getattr(eng.lib, f"pp_{fam}_backward_{form}_mp")(eng.ctx, mode, *ints, *[ptr(t) for t in (*pre, *normd, *post)], nb, *[ptr(t) for t in outs],
                                                          *tail, None)
    torch.cuda.synchronize()
    return outs, rc


# ------------------------------------------------------------------ 1. mode 0 is the old call
@pytest.mark.parametrize("form", R.FORMS)
def test_mode0_is_the_fp32_entry(form):
    eng = engine()
    shape = R.UNIT_SHAPES[1]
    _, (ud, wd, normd, dzd, dsd), _ = unit_set(shape, form)
    old = (eng.unit_backward_affine if form == "affine" else eng.unit_backward_bn)(ud, wd, *normd, dzd, dskip=dsd)
    outs, rc = c_entry(eng, "unit", 0, shape[:3], (ud, wd), normd, (dzd, dsd), shape[3], (tuple(wd.shape), tuple(ud.shape)))
    assert rc == 0 and same(old, unit(eng, ud, wd, normd, dzd, "fp32", dskip=dsd)) and same(old, outs)
    shape = S.DOWN_SHAPES[1]
    _, (xd, wd, zd, normd, dyd), _ = down_set(shape, form)
    old = (eng.down_backward_affine if form == "affine" else eng.down_backward_bn)(xd, wd, zd, *normd, dyd)
    outs, rc = c_entry(eng, "down", 0, shape[:4], (xd, wd, zd), normd, (dyd,), shape[4], (tuple(wd.shape), tuple(xd.shape)))
    assert rc == 0 and same(old, down(eng, xd, wd, zd, normd, dyd, "fp32")) and same(old, outs)
    H, W, nb = S.NECK_MAPS[0]
    eng = engine(2 * H, 2 * W)
    _, (xs, ws, norms, yd, dyd), _ = neck_set(S.NECK_MAPS[0], form)
    for b in range(3):
        old = (eng.neck_backward_affine if form == "affine" else eng.neck_backward_bn)(b, xs[b], ws[b], *norms[b], yd, dyd)
        outs, rc = c_entry(eng, "neck", 0, (b,), (xs[b], ws[b]), norms[b], (yd, dyd), nb, (tuple(ws[b].shape), tuple(xs[b].shape)))
        assert rc == 0 and same(old, neck(eng, b, xs[b], ws[b], norms[b], yd, dyd, "fp32")) and same(old, outs)
    assert eng.unit_backward_path("fp32", 64, 9, 9, bn=True) == eng.down_backward_path("fp32", 64, 64, 9, 9, bn=True) == "fp32"
    assert eng.neck_backward_path("fp32", 1, bn=True) == "fp32"


# ------------------------------------------------------------------ 2. and 3. shapes, and what the mode may not touch
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("shape", R.UNIT_SHAPES + [R.UNIT_LARGE])
def test_unit_shapes(shape, form):
    eng = engine()
    (u, w, norm, dz, dskip), (ud, wd, normd, dzd, dsd), t = unit_set(shape, form)
    fp32 = unit(eng, ud, wd, normd, dzd, "fp32", dskip=dsd)
    for mode in MODES:
        assert eng.unit_backward_path(mode, *shape[:3], bn=True) == mode
        got = unit(eng, ud, wd, normd, dzd, mode)
        check(got, *R.unit_bounds_mixed(u, w, norm, dz, mode, terms=t), f"unit {form} {shape} {mode}")
        assert same(got, unit(eng, ud, wd, normd, dzd, mode))  # two runs
        dw3, none, ds3, dh3 = unit(eng, ud, wd, normd, dzd, mode, need_du=False, need_affine=False)
        assert none is None and ds3 is None and dh3 is None and torch.equal(dw3, got[0])
        skip = unit(eng, ud, wd, normd, dzd, mode, dskip=dsd)
        assert torch.equal(skip[0], got[0]) and torch.equal(skip[1], got[1] + dsd) and same(skip[2:], got[2:])  # dskip is exactly one fp32 add
        check(skip, *R.unit_bounds_mixed(u, w, norm, dz, mode, dskip=dskip, terms=t), f"unit {form} {shape} {mode} + dskip")
        if form == "affine":  # the mask is the fp32 one: where the fp32 entry's du is exactly dskip (masked out), so is the twin's
            out = fp32[1] == dsd
            assert 0.2 < float(out.float().mean()) < 0.8 and torch.equal(skip[1][out], dsd[out])


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("shape", S.DOWN_SHAPES)
def test_down_shapes(shape, form):
    eng = engine()
    _, (xd, wd, zd, normd, dyd), t = down_set(shape, form)
    fp32 = down(eng, xd, wd, zd, normd, dyd, "fp32")
    for mode in MODES:
        assert eng.down_backward_path(mode, *shape[:4], bn=True) == mode
        got = down(eng, xd, wd, zd, normd, dyd, mode)
        check(got, *R.stage_bounds_mixed(t, mode), f"down {form} {shape} {mode}")
        assert torch.equal(got[2], fp32[2]) and torch.equal(got[3], fp32[3])  # dscale, dshift: the fp32 path's bits
        assert same(got, down(eng, xd, wd, zd, normd, dyd, mode))
        dw3, none, ds3, dh3 = down(eng, xd, wd, zd, normd, dyd, mode, need_dx=False)
        assert none is None and torch.equal(dw3, got[0]) and torch.equal(ds3, got[2]) and torch.equal(dh3, got[3])


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("shape", S.NECK_MAPS)
def test_neck_shapes(shape, form):
    H, W, nb = shape
    eng = engine(2 * H, 2 * W)
    _, (xs, ws, norms, yd, dyd), terms = neck_set(shape, form)
    for b in range(3):
        fp32 = neck(eng, b, xs[b], ws[b], norms[b], yd, dyd, "fp32")
        for mode in MODES:
            assert eng.neck_backward_path(mode, b, bn=True) == mode
            got = neck(eng, b, xs[b], ws[b], norms[b], yd, dyd, mode)
            check(got, *R.stage_bounds_mixed(terms[b], mode), f"neck {form} {shape} branch {b} {mode}")
            assert torch.equal(got[2], fp32[2]) and torch.equal(got[3], fp32[3])
            assert same(got, neck(eng, b, xs[b], ws[b], norms[b], yd, dyd, mode))
            dw3, none, ds3, dh3 = neck(eng, b, xs[b], ws[b], norms[b], yd, dyd, mode, need_dx=False)
            assert none is None and torch.equal(dw3, got[0]) and torch.equal(ds3, got[2]) and torch.equal(dh3, got[3])


# ------------------------------------------------------------------ 4. exact data: every mode computes the fp32 entry's bits
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("shape", R.EXACT_UNITS)
def test_exact_unit(shape, form):
    eng = engine()
    u, w, norm, dz = R.exact_unit(*shape, form)
    ud, wd, normd, dzd = dev(u), dev(w), devs(norm), dev(dz)
    fp32 = unit(eng, ud, wd, normd, dzd, "fp32")
    assert float(fp32[0].abs().max()) > 0 and float(fp32[1].abs().max()) > 0
    for mode in MODES:
        got = unit(eng, ud, wd, normd, dzd, mode)
        for name, a, b in zip(("dw", "du", "dscale", "dshift"), got, fp32):
            assert torch.equal(a, b), (shape, form, mode, name, int((a != b).sum()), float((a - b).abs().max()))


@pytest.mark.parametrize("shape", R.EXACT_DOWNS)
def test_exact_down(shape):
    eng = engine()
    x, w, z, norm, dy = R.exact_down(*shape)
    xd, wd, zd, normd, dyd = dev(x), dev(w), dev(z), devs(norm), dev(dy)
    fp32 = down(eng, xd, wd, zd, normd, dyd, "fp32")
    for mode in MODES:
        got = down(eng, xd, wd, zd, normd, dyd, mode)
        assert same(got, fp32), (shape, mode, [int((a != b).sum()) for a, b in zip(got, fp32)])
    # the batch form's dz is not dyadic: it is held to its bound
    x, w, z, norm, dy = R.exact_down(*shape, form="batch")
    t = R.down_terms(x, w, z, norm, dy)
    for mode in MODES:
        check(down(eng, dev(x), dev(w), dev(z), devs(norm), dev(dy), mode), *R.stage_bounds_mixed(t, mode), f"exact down batch {shape} {mode}")


def test_exact_neck():
    H, W, nb = R.EXACT_NECK
    eng = engine(2 * H, 2 * W)
    for form in R.FORMS:
        xs, ws, norms, y, dy = R.exact_neck(H, W, nb, form)
        yd, dyd = dev(y), dev(dy)
        for b in range(3):
            xd, wd, normd = dev(xs[b]), dev(ws[b]), devs(norms[b])
            sl = S.branch_slice(b)
            for mode in MODES:
                got = neck(eng, b, xd, wd, normd, yd, dyd, mode)
                if form == "affine":
                    fp32 = neck(eng, b, xd, wd, normd, yd, dyd, "fp32")
                    assert same(got, fp32), (b, mode, [int((a != c).sum()) for a, c in zip(got, fp32)])
                else:
                    t = R.neck_terms(xs[b], ws[b], norms[b], y[:, sl], dy[:, sl])
                    check(got, *R.stage_bounds_mixed(t, mode), f"exact neck batch branch {b} {mode}")


# ------------------------------------------------------------------ 5. frames and chunks
@pytest.mark.parametrize("mode", MODES)
def test_affine_frames(mode):
    """A frame's du / dx inside a 3-frame call equals the same frame alone."""
    eng = engine()
    _, (ud, wd, normd, dzd, dsd), _ = unit_set(R.UNIT_SHAPES[2], "affine")
    du = unit(eng, ud, wd, normd, dzd, mode, dskip=dsd)[1]
    _, (xd, wdd, zd, normdd, dyd), _ = down_set(S.DOWN_SHAPES[2], "affine")
    dx = down(eng, xd, wdd, zd, normdd, dyd, mode)[1]
    assert ud.shape[0] == xd.shape[0] == 3
    for f in range(3):
        s = slice(f, f + 1)
        assert torch.equal(unit(eng, ud[s].contiguous(), wd, normd, dzd[s].contiguous(), mode, dskip=dsd[s].contiguous())[1][0], du[f]), f
        assert torch.equal(down(eng, xd[s].contiguous(), wdd, zd[s].contiguous(), normdd, dyd[s].contiguous(), mode)[1][0], dx[f]), f
    H, W, nb = S.NECK_MAPS[0]
    eng = engine(2 * H, 2 * W)
    _, (xs, ws, norms, yd, dyd), _ = neck_set(S.NECK_MAPS[0], "affine")
    assert nb == 3
    for b in range(3):
        dx = neck(eng, b, xs[b], ws[b], norms[b], yd, dyd, mode)[1]
        for f in range(3):
            s = slice(f, f + 1)
            assert torch.equal(neck(eng, b, xs[b][s].contiguous(), ws[b], norms[b], yd[s].contiguous(), dyd[s].contiguous(), mode)[1][0], dx[f]), (b, f)


@pytest.mark.parametrize("mode", MODES)
def test_batch_chunks(mode):
    """chunk_frames 1 and 2 against the workspace rule, as an argument and through pp_set_train_chunk_frames: du / dx and the sums keep
    their bits, dw stays inside its bound (nb = 3)."""
    eng = engine()
    (u, w, norm, dz, dskip), (ud, wd, normd, dzd, dsd), tu = unit_set(R.UNIT_SHAPES[2], "batch")
    _, (xd, wdd, zd, normdd, dyd), td = down_set(S.DOWN_SHAPES[2], "batch")
    H, W, nb = S.NECK_MAPS[0]
    neng = engine(2 * H, 2 * W)
    _, (xs, ws, norms, yd, dyyd), tn = neck_set(S.NECK_MAPS[0], "batch")
    calls = [("unit", eng, lambda k: unit(eng, ud, wd, normd, dzd, mode, dskip=dsd, chunk_frames=k),
              R.unit_bounds_mixed(u, w, norm, dz, mode, dskip=dskip, terms=tu)),
             ("down", eng, lambda k: down(eng, xd, wdd, zd, normdd, dyd, mode, chunk_frames=k), R.stage_bounds_mixed(td, mode))]
    calls += [(f"neck {b}", neng, lambda k, b=b: neck(neng, b, xs[b], ws[b], norms[b], yd, dyyd, mode, chunk_frames=k), R.stage_bounds_mixed(tn[b], mode))
              for b in range(3)]
    for what, e, call, (want, bounds) in calls:
        base = call(0)
        for k in (1, 2):
            got = call(k)
            assert same(got[1:], base[1:]), (what, k)
            check_bound(got[0], want[0], bounds[0], f"{what} {mode} dw, chunk_frames {k}")
            try:
                e.set_train_chunk_frames(k)
                capped = call(0)
            finally:
                e.set_train_chunk_frames(0)
            assert same(capped, got), (what, k)  # the context's cap is the argument's
        assert same(call(0), base)


# ------------------------------------------------------------------ 6. path queries
@pytest.mark.parametrize("norm", ("instance", "batch"))
def test_path_queries(norm):
    eng = engine(norm=norm)
    for mode in MODES:
        for C, h, w in [s[:3] for s in R.UNIT_SHAPES + [R.UNIT_LARGE] + R.EXACT_UNITS] + NETWORK_UNITS:
            assert eng.unit_backward_path(mode, C, h, w, bn=True) == mode, (mode, C, h, w)
        for s in [s[:4] for s in S.DOWN_SHAPES + R.EXACT_DOWNS] + NETWORK_DOWNS:
            assert eng.down_backward_path(mode, *s, bn=True) == mode, (mode, s)
        for b in range(3):
            assert eng.neck_backward_path(mode, b, bn=True) == mode
    # 640 x 640 at C = 64: the hi and lo images of one frame pass the 256 MB budget: the fp32 kernels run
    assert eng.unit_backward_path("bf16x3", 64, 640, 640, bn=True) == "fp32" and eng.unit_backward_path("bf16", 64, 640, 640, bn=True) == "bf16"
    with pytest.raises(ValueError):
        eng.unit_backward_path("fp8", 64, 10, 10, bn=True)
    for bad in ((96, 10, 10), (64, 1, 1)):
        with pytest.raises(RuntimeError, match="pp_unit_backward_bn_path"):
            eng.unit_backward_path("bf16", *bad, bn=True)
    with pytest.raises(RuntimeError, match="pp_down_backward_bn_path"):
        eng.down_backward_path("bf16", 96, 96, 10, 10, bn=True)
    with pytest.raises(RuntimeError, match="pp_down_backward_bn_path"):
        eng.down_backward_path("bf16", 64, 64, 1, 1, bn=True)
    with pytest.raises(ValueError):
        eng.neck_backward_path("bf16", 3, bn=True)
    lib = eng.lib
    for mode in (3, -1):
        assert lib.pp_unit_backward_bn_path(eng.ctx, mode, 64, 10, 10) < 0 and b"pp_unit_backward_bn_path: mode" in lib.pp_last_error(eng.ctx)
        assert lib.pp_down_backward_bn_path(eng.ctx, mode, 64, 64, 10, 10) < 0 and b"pp_down_backward_bn_path: mode" in lib.pp_last_error(eng.ctx)
        assert lib.pp_neck_backward_bn_path(eng.ctx, mode, 0) < 0 and b"pp_neck_backward_bn_path: mode" in lib.pp_last_error(eng.ctx)
    assert lib.pp_neck_backward_bn_path(eng.ctx, 1, 3) < 0
    if norm == "batch":  # the existing queries keep refusing a BatchNorm context
        with pytest.raises(RuntimeError):
            eng.unit_backward_path("bf16", 64, 10, 10)


# ------------------------------------------------------------------ 7. the modes are told apart
def test_modes_are_told_apart():
    eng = engine()
    (u, w, norm, dz, _), (ud, wd, normd, dzd, _), _ = unit_set(R.UNIT_APART, "affine")
    (rw, _, _, _), (bw, _, _, _) = RA.unit_bounds(u, w, *norm, dz)
    dev_ = {mode: np.abs(unit(eng, ud, wd, normd, dzd, mode)[0].cpu().numpy().astype(np.float64) - rw) for mode in MODES}
    print(f"bf16 dw: {float((dev_['bf16'] / bw).max()):.2f} of the plain fp32 bound; largest deviations bf16 {dev_['bf16'].max():.3e}, "
          f"bf16x3 {dev_['bf16x3'].max():.3e}")
    assert (dev_["bf16"] / bw).max() > 1.0  # plain bf16 leaves the fp32 bound: the 16-bit kernels ran
    assert dev_["bf16x3"].max() < dev_["bf16"].max() / 16


# ------------------------------------------------------------------ 8. the autograd surface
def record(net, monkeypatch):
    eng, seen = net._eng, []
    inner = {"unit": eng.unit_backward, "down": eng.down_backward, "neck": eng.neck_backward}

    def rec(family):
        def call(*args, **kw):
            out = inner[family](*args, **kw)
            seen.append((family, args, kw, out))
            return out
        return call

    for family in inner:
        monkeypatch.setattr(eng, family + "_backward", rec(family))
    return seen


def call_bounds(family, args, kw, mode):
    """The bound of one recorded call from its own inputs."""
    n64 = lambda *ts: [t.detach().cpu().numpy() for t in ts]  # noqa: E731
    norm = kw["norm"]
    nt = tuple(n64(*[t for t in (norm.scale, norm.shift, norm.mean, norm.var) if t is not None]))
    if family == "unit":
        u, w, dz = n64(*args[:3])
        dskip = None if kw.get("dskip") is None else n64(kw["dskip"])[0]
        return R.unit_bounds_mixed(u, w, nt, dz, mode, dskip=dskip)
    if family == "down":
        x, w, z, dy = n64(*args[:4])
        return R.stage_bounds_mixed(R.down_terms(x, w, z, nt, dy), mode)
    b = args[0]
    x, w, y, dy = n64(*args[1:5])
    sl = S.branch_slice(b)
    return R.stage_bounds_mixed(R.neck_terms(x, w, nt, y[:, sl], dy[:, sl]), mode)


@pytest.mark.parametrize("stats", ("frozen", "moving"))
def test_autograd_surface(stats, monkeypatch):
    load_pkg().install()
    net, sd, canvas, ws, bn, dy = fixture_net()
    assert tuple(canvas.shape) == (2, 64, 32, 24)
    cv, dyd = dev(canvas), dev(dy)
    seen = record(net, monkeypatch)

    def grads_of(**kw):
        net.load_state_dict(sd)  # the running statistics move under "moving": every run starts from the fixture's
        net.train(scope="rpn", bn_stats=stats, **kw)
        net.zero_grad()
        del seen[:]
        net.rpn_train(cv).backward(dyd)
        grads = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
        return grads, list(seen)

    base, base_calls = grads_of()
    assert len(base) == 57 and len(base_calls) == 19 and all("bn_grad_precision" not in c[2] and "grad_precision" not in c[2] for c in base_calls)
    explicit, calls = grads_of(bn_grad_precision="fp32")
    assert all("bn_grad_precision" not in c[2] for c in calls) and all(torch.equal(base[k], explicit[k]) for k in base)
    mode = "bf16x3" if stats == "frozen" else "bf16"  # one mode per form: the bound of every call is evaluated from its own inputs
    for stages in ("units", "rpn"):
        got, calls = grads_of(bn_grad_precision=mode, grad_stages=stages)
        assert (net.bn_grad_precision, net.grad_stages, net.grad_precision) == (mode, stages, "fp32")
        assert len(calls) == 19 and len(got) == 57 and all(torch.isfinite(g).all() for g in got.values())
        for family, args, kw, out in calls:
            promised = mode if family == "unit" or stages == "rpn" else None
            assert kw.get("bn_grad_precision") == promised and "grad_precision" not in kw, (family, kw.keys())
            assert (kw["norm"].mean is None) == (stats == "frozen")
            if stages == "rpn" or family == "unit":
                want, bounds = call_bounds(family, args, kw, promised or "fp32")
                names = [n for n, o in zip(("dw", "dx", "dscale", "dshift"), out) if o is not None]
                keep = [i for i, o in enumerate(out) if o is not None]
                check([out[i] for i in keep], [want[i] for i in keep], [bounds[i] for i in keep], f"{stats} {stages} {family}", names)
        if stages == "units":  # the upsamplers run first and stay fp32: their gradients are the fp32 run's bits
            shared = load_pkg("networks.pointpillars8_shared")
            assert all(torch.equal(got[k], base[k]) for k in shared.NECK_KEYS)
    net.eval()
    assert net.bn_grad_precision == "fp32"


# ------------------------------------------------------------------ 9. it trains
@pytest.mark.parametrize("mode", ("fp32",) + MODES)
def test_it_trains(mode):
    """Twenty Adam steps (lr 1e-3, clip_grad_norm_ 10) on a fixed batch of two frames under scope "rpn", bn_stats="moving",
    grad_stages="rpn".  A sanity condition, not a measurement: a mode that cannot halve the loss is not training."""
    load_pkg().install()
    LossGenerator = load_pkg("framework.loss_generator").LossGenerator
    net, cfg = bn_net()
    eng = net._eng
    example = two_frames(eng)
    rng = np.random.default_rng(21)
    u = rng.random((2, eng.A))
    labels = np.where(u < 1 / 7, 1, np.where(u < 0.75, 0, -1)).astype(np.int32)
    ex = {"labels": labels, "bbox_targets": (rng.standard_normal((2, eng.A, 7)) * 0.4).astype(np.float32) * (labels > 0)[..., None],
          "dir_targets": (rng.random((2, eng.A)) < 0.5).astype(np.int32)}
    lg = LossGenerator(cfg)
    net.train(scope="rpn", bn_stats="moving", bn_grad_precision=mode, grad_stages="rpn")
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    losses = []
    for _ in range(20):
        loss = lg.generate(net(example), ex)["loss"]
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(net.parameters()), 10.0)
        opt.step()
        losses.append(float(loss))
    with torch.no_grad():
        losses.append(float(lg.generate(net(example), ex)["loss"]))
    print(mode, " ".join(f"{v:.6f}" for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < 0.5 * losses[0], (mode, losses)
    net.eval()
    assert net.bn_grad_precision == "fp32" and not net.training
    with torch.no_grad():
        out = net(example)
    assert all(torch.isfinite(v).all() for v in out.values())


# ------------------------------------------------------------------ 10. errors
@pytest.mark.parametrize("form", R.FORMS)
def test_refused_calls_name_the_entry_and_the_next_call_works(form):
    eng = engine()
    suffix = "affine" if form == "affine" else "bn"
    last = lambda: eng.lib.pp_last_error(eng.ctx).decode()  # noqa: E731
    shape = (64, 9, 7, 2)
    u, w, norm, dz, _ = R.unit_case(*shape, form)
    ud, wd, normd, dzd = dev(u), dev(w), devs(norm), dev(dz)
    good = unit(eng, ud, wd, normd, dzd, "bf16")
    sh = (tuple(wd.shape), tuple(ud.shape))
    unit_c = lambda mode, normd=normd, nb=2: c_entry(eng, "unit", mode, shape[:3], (ud, wd), normd, (dzd, None), nb, sh)  # noqa: E731
    dshape = (64, 64, 9, 7, 2)
    x, wdn, z, dnorm, dy = R.down_case(*dshape, form)
    xd, wdd, zd, dnormd, dyd = dev(x), dev(wdn), dev(z), devs(dnorm), dev(dy)
    dgood = down(eng, xd, wdd, zd, dnormd, dyd, "bf16")
    dsh = (tuple(wdd.shape), tuple(xd.shape))
    down_c = lambda mode, normd=dnormd, nb=2: c_entry(eng, "down", mode, dshape[:4], (xd, wdd, zd), normd, (dyd,), nb, dsh)  # noqa: E731
    xs, ws, norms, y, dyn = R.neck_case(12, 8, 2, form)
    nxd, nwd, nnormd, yd, dynd = dev(xs[1]), dev(ws[1]), devs(norms[1]), dev(y), dev(dyn)
    ngood = neck(eng, 1, nxd, nwd, nnormd, yd, dynd, "bf16")
    nsh = (tuple(nwd.shape), tuple(nxd.shape))
    neck_c = lambda mode, normd=nnormd, nb=2: c_entry(eng, "neck", mode, (1,), (nxd, nwd), normd, (yd, dynd), nb, nsh)  # noqa: E731
    for fam, call in (("unit", unit_c), ("down", down_c), ("neck", neck_c)):
        name = f"pp_{fam}_backward_{suffix}"
        for mode in (3, -1):
            assert call(mode)[1] != 0 and last().startswith(name + "_mp: mode"), last()
        for mode in (0, 1, 2):
            null_scale = [None] + list({"unit": normd, "down": dnormd, "neck": nnormd}[fam][1:])
            assert call(mode, normd=null_scale)[1] != 0 and name in last() and "null" in last(), last()
            assert call(mode, nb=4)[1] != 0 and name in last() and "max_batch" in last(), last()
    # dscale without du
    C = 64
    dw, ds, dh = torch.empty_like(wd), torch.empty(C, device="cuda", dtype=torch.float64), torch.empty(C, device="cuda", dtype=torch.float64)
    tail = [0] if form == "batch" else []
    for mode in (0, 1, 2):
        rc = getattr(eng.lib, f"pp_unit_backward_{suffix}_mp")(eng.ctx, mode, *shape[:3], ptr(ud), ptr(wd), *[ptr(t) for t in normd], ptr(dzd), None, 2,
                                                              ptr(dw), None, ptr(ds), ptr(dh), *tail, None)
        assert rc != 0 and f"pp_unit_backward_{suffix}" in last() and "need du" in last(), last()
    # the next good call works, and computes what it computed
    for call, want in ((unit_c, good), (down_c, dgood), (neck_c, ngood)):
        outs, rc = call(2)
        assert rc == 0 and same(outs, want)
    assert same(unit(eng, ud, wd, normd, dzd, "bf16"), good)
