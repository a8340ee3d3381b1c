"""GPU: the frame-chunked paths of every training backward.  Each of pp_{unit,down,neck}_backward, its _affine form and its _mp form
in modes 1 and 2 (twelve chunk loops in csrc/{block,down,neck}_train{,16}.hip) walks the batch in chunks of fc frames, and fc comes
from a byte budget that no test map comes near: without help every test runs one chunk.  pp_set_train_chunk_frames caps fc for a whole
context, so the smallest shapes of the sibling test files run 1 + 1 + 1, 2 + 1 and 2 + 2 + 1 frames here.

Nothing new is taken for a reference or a tolerance.  Inputs come from the case makers of the sibling files, the float64 references and
element-wise a-priori bounds from blocktrain_ref / mixedtrain_ref (units), mixedstage_ref over downtrain_ref and necktrain_ref (strided
stages, upsamplers; its "fp32" terms are those modules' own grad_bounds), bntrain_ref (affine) and, for the three _bn entries,
test_bnbatch_gpu.chunks_agree over bnbatch_ref.  Per loop and shape:
  inert     caps 0, nb and nb + 1 give every output bit-equal to an engine whose setter was never called;
  chunked   caps 1 and 2 leave du / dx (with dskip too) and the affine sums bit-equal to that engine's, and dw inside the a-priori bound
            of the uncapped call.  dw's bits may move, because the K ranges follow the chunks, and need not: on a map this small a range
            is often a single chunk of positions, and the reduce kernel adds the partials in double.  test_setter uses a case where they
            do move, so a cap that stopped reaching the loops fails there;
  pieces    the capped dw against the sum of the uncapped calls on each chunk's frames: dw_ranges depends on the tiles and on fn x cpf
            alone, so the capped call forms the same partials, adds them in double and rounds once where the pieces round once each:
            |dw - sum dw_i| <= 1.01 x 2^-24 x (|dw| + sum |dw_i|), element-wise in float64;
  flags     need_dx / need_du = False and a repeated call keep dw's bits under the cap;
  raw       the C entry itself at cap 1 into NaN-filled dw and dx / du is the wrapper's result: nothing is left unwritten.
No output of the twelve loops other than dw was found to depend on the chunking."""
import ctypes
import functools
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden, load_pkg
import blocktrain_ref as B
import bnbatch_ref as BB
import bntrain_ref as A
import mixedstage_ref as S
import mixedtrain_ref as M
import rpntrain_ref as RR
from train_common import check_bound, check_grad, dev, small_cfg
from test_bnbatch_gpu import chunks_agree, folded32
from test_bntrain_gpu import bn_net, bn_sd, down_case as affine_down_case, norm_params, same, unit_case as affine_unit_case
from test_mixedtrain_gpu import random_case as unit_case

sys.path.insert(0, GOLDEN)
import make_bntrain_goldens as GB  # noqa: E402
import make_rpntrain_goldens as GR  # noqa: E402

pytestmark = pytest.mark.gpu
ENG = load_pkg("engine").Engine
KINDS = ("fp32", "affine", "bf16x3", "bf16")  # the four loops of a family
ENTRY = {"fp32": "backward", "affine": "backward_affine", "bf16x3": "backward_mp mode 1 (bf16x3)", "bf16": "backward_mp mode 2 (bf16)"}
H, W = 40, 24                                  # the level-0 map of the upsampler cases
UNIT_SHAPES = [(64, 33, 17), (128, 20, 18), (256, 3, 2)]
DOWN_SHAPES = [(64, 64, 33, 18), (64, 128, 40, 26), (128, 256, 25, 9)]
U24 = 2.0 ** -24
_ENGINES = {}


def engine(which):
    """Two engines of one geometry (80 x 48 cells, max_batch 5) without weights: every entry here is stateless.  "capped" is the one
    whose cap the tests move; "pristine" never sees the setter and makes every uncapped call."""
    if which not in _ENGINES:
        load_pkg().install()
        _ENGINES[which] = ENG(small_cfg(2 * H, 2 * W, 5))
    return _ENGINES[which]


@pytest.fixture(autouse=True)
def cap_back_to_zero():
    yield
    for which, eng in _ENGINES.items():
        if which != "pristine":
            eng.set_train_chunk_frames(0)


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def outs(t):
    """The outputs a call returned, without the ones it was told to skip."""
    return [x for x in t if x is not None]


class Loop:
    """One chunk loop at one case: call(eng, frames, dskip, need_dx) through the wrapper, ref() -> the float64 dw and its bound, raw(eng,
    dw, dx, sums) -> the C entry's return code."""

    def __init__(self, name, nb, call, ref, raw, has_dskip=False):
        self.name, self.nb, self.call, self.raw, self.has_dskip = name, nb, call, raw, has_dskip
        self.ref = functools.lru_cache(maxsize=None)(ref)


@functools.lru_cache(maxsize=None)
def unit_loop(kind, C, h, w, nb):
    name = f"pp_unit_{ENTRY[kind]} {C}x{h}x{w}x{nb}"
    if kind == "affine":
        u, wt, (sc, sh), dz, dskip = affine_unit_case(C, h, w, nb, 200 + C + h)
        ud, wd, scd, shd, dzd, dsd = (dev(t) for t in (u, wt, sc, sh, dz, dskip))

        def call(eng, fr=slice(None), dskip=False, need_dx=True):
            return eng.unit_backward_affine(ud[fr], wd, scd, shd, dzd[fr], dskip=dsd[fr] if dskip else None, need_du=need_dx, need_affine=need_dx)

        def ref():
            want, bounds = A.unit_bounds(u, wt, sc, sh, dz)
            return want[0], bounds[0]

        def raw(eng, dw, du, sums):
            return eng.lib.pp_unit_backward_affine(eng.ctx, C, h, w, ptr(ud), ptr(wd), ptr(scd), ptr(shd), ptr(dzd), None, nb, ptr(dw), ptr(du),
                                                   ptr(sums[0]), ptr(sums[1]), None)
    else:
        u, wt, dz, dskip = unit_case(C, h, w, nb, 100 + C + h)
        ud, wd, dzd, dsd = (dev(t) for t in (u, wt, dz, dskip))

        def call(eng, fr=slice(None), dskip=False, need_dx=True):
            return eng.unit_backward(ud[fr], wd, dzd[fr], dskip=dsd[fr] if dskip else None, need_du=need_dx, grad_precision=kind)

        def ref():
            rw, _, bw, _, ties = B.grad_bounds(u, wt, dz) if kind == "fp32" else M.grad_bounds_mixed(u, wt, dz, kind)
            assert not ties.any()
            return rw, bw

        def raw(eng, dw, du, sums):
            if kind == "fp32":
                return eng.lib.pp_unit_backward(eng.ctx, C, h, w, ptr(ud), ptr(wd), ptr(dzd), None, nb, ptr(dw), ptr(du), None)
            return eng.lib.pp_unit_backward_mp(eng.ctx, ENG.GRAD_PRECISIONS[kind], C, h, w, ptr(ud), ptr(wd), ptr(dzd), None, nb, ptr(dw), ptr(du), None)
    return Loop(name, nb, call, ref, raw, has_dskip=True)


@functools.lru_cache(maxsize=None)
def down_terms(shape, nb):
    case = S.down_case(*shape, nb)
    t = S.down_terms(*case)
    assert not t["ties"].any()
    return case, t


@functools.lru_cache(maxsize=None)
def down_loop(kind, shape, nb):
    cin, cout, hin, win = shape
    name = f"pp_down_{ENTRY[kind]} {cin}->{cout} {hin}x{win}x{nb}"
    if kind == "affine":
        x, wt, z, (sc, sh), dy = affine_down_case(cin, cout, hin, win, nb, 300 + cout + hin)
        xd, wd, zd, scd, shd, dyd = (dev(t) for t in (x, wt, z, sc, sh, dy))

        def call(eng, fr=slice(None), dskip=False, need_dx=True):
            return eng.down_backward_affine(xd[fr], wd, zd[fr], scd, shd, dyd[fr], need_dx=need_dx)

        def ref():
            want, bounds = A.down_bounds(x, wt, z, sc, sh, dy)
            return want[0], bounds[0]

        def raw(eng, dw, dx, sums):
            return eng.lib.pp_down_backward_affine(eng.ctx, cin, cout, hin, win, ptr(xd), ptr(wd), ptr(zd), ptr(scd), ptr(shd), ptr(dyd), nb, ptr(dw),
                                                   ptr(dx), ptr(sums[0]), ptr(sums[1]), None)
    else:
        (x, wt, z, dy), _ = down_terms(shape, nb)
        xd, wd, zd, dyd = (dev(t) for t in (x, wt, z, dy))

        def call(eng, fr=slice(None), dskip=False, need_dx=True):
            return eng.down_backward(xd[fr], wd, zd[fr], dyd[fr], need_dx=need_dx, grad_precision=kind)

        def ref():
            case, t = down_terms(shape, nb)
            rw, _, bw, _, _ = S.down_grad_bounds_mixed(*case, kind, terms=t)  # "fp32": downtrain_ref.grad_bounds itself
            return rw, bw

        def raw(eng, dw, dx, sums):
            if kind == "fp32":
                return eng.lib.pp_down_backward(eng.ctx, cin, cout, hin, win, ptr(xd), ptr(wd), ptr(zd), ptr(dyd), nb, ptr(dw), ptr(dx), None)
            return eng.lib.pp_down_backward_mp(eng.ctx, ENG.GRAD_PRECISIONS[kind], cin, cout, hin, win, ptr(xd), ptr(wd), ptr(zd), ptr(dyd), nb, ptr(dw),
                                               ptr(dx), None)
    return Loop(name, nb, call, ref, raw)


@functools.lru_cache(maxsize=None)
def neck_inputs(nb):
    xs, ws, y, dy = S.neck_case(H, W, nb)
    return xs, ws, y, dy, dev(y), dev(dy)


@functools.lru_cache(maxsize=None)
def neck_terms(branch, nb):
    xs, ws, y, dy, _, _ = neck_inputs(nb)
    sl = S.branch_slice(branch)
    case = (xs[branch], ws[branch], y[:, sl], dy[:, sl])
    return case, S.neck_terms(*case)


@functools.lru_cache(maxsize=None)
def neck_loop(kind, branch, nb):
    name = f"pp_neck_{ENTRY[kind]} branch {branch} {H}x{W}x{nb}"
    if kind == "affine":  # the case of test_bntrain_gpu.test_neck on this map
        rng = np.random.default_rng(400 + branch)
        cin, cup, coff, s = A.N.CIN[branch], A.N.CUP[branch], A.N.COFF[branch], 1 << branch
        x = rng.standard_normal((nb, cin, H >> branch, W >> branch)).astype(np.float32)
        wt = (rng.standard_normal((cin, cup, s, s)) * 0.05).astype(np.float32)
        sc, sh = A.fold32(*norm_params(rng, cup))
        y = rng.standard_normal((nb, 320, H, W)).astype(np.float32)  # the mask is the given y, whatever the forward would give
        y[:, coff:coff + cup] = np.maximum(A.aff(A.N.conv_t(x, wt), sc, sh), 0.0).astype(np.float32)
        y[0, coff, 0, :3] = (0.0, 1.0, 0.0)  # and not a recomputed sign
        dy = rng.standard_normal(y.shape).astype(np.float32)
        xd, wd, scd, shd, yd, dyd = (dev(t) for t in (x, wt, sc, sh, y, dy))

        def call(eng, fr=slice(None), dskip=False, need_dx=True):
            return eng.neck_backward_affine(branch, xd[fr], wd, scd, shd, yd[fr], dyd[fr], need_dx=need_dx)

        def ref():
            sl = slice(coff, coff + cup)
            want, bounds = A.branch_backward(x, wt, sc, y[:, sl], dy[:, sl], bounds=True)
            return want[0], bounds[0]

        def raw(eng, dw, dx, sums):
            return eng.lib.pp_neck_backward_affine(eng.ctx, branch, ptr(xd), ptr(wd), ptr(scd), ptr(shd), ptr(yd), ptr(dyd), nb, ptr(dw), ptr(dx),
                                                   ptr(sums[0]), ptr(sums[1]), None)
    else:
        xs, ws, _, _, yd, dyd = neck_inputs(nb)
        xd, wd = dev(xs[branch]), dev(ws[branch])

        def call(eng, fr=slice(None), dskip=False, need_dx=True):
            return eng.neck_backward(branch, xd[fr], wd, yd[fr], dyd[fr], need_dx=need_dx, grad_precision=kind)

        def ref():
            case, t = neck_terms(branch, nb)
            rw, _, bw, _ = S.neck_grad_bounds_mixed(*case, kind, terms=t)  # "fp32": necktrain_ref.grad_bounds itself
            return rw, bw

        def raw(eng, dw, dx, sums):
            if kind == "fp32":
                return eng.lib.pp_neck_backward(eng.ctx, branch, ptr(xd), ptr(wd), ptr(yd), ptr(dyd), nb, ptr(dw), ptr(dx), None)
            return eng.lib.pp_neck_backward_mp(eng.ctx, ENG.GRAD_PRECISIONS[kind], branch, ptr(xd), ptr(wd), ptr(yd), ptr(dyd), nb, ptr(dw), ptr(dx), None)
    return Loop(name, nb, call, ref, raw)


def loop_of(family, kind, shape, nb):
    return {"unit": lambda: unit_loop(kind, *shape, nb), "down": lambda: down_loop(kind, shape, nb), "neck": lambda: neck_loop(kind, shape, nb)}[family]()


CASES = [("unit", s) for s in UNIT_SHAPES] + [("down", s) for s in DOWN_SHAPES] + [("neck", b) for b in range(3)]
FIVE = [("unit", (128, 20, 18)), ("down", (128, 256, 25, 9)), ("neck", 1)]  # one shape per family at 2 + 2 + 1 frames


def case_id(v):
    return v if isinstance(v, str) else "x".join(str(i) for i in v) if isinstance(v, tuple) else f"branch{v}"


def pieces_agree(dw, parts, what):
    """The capped dw against the uncapped calls on each chunk's frames (module docstring, "pieces")."""
    d = dw.cpu().numpy().astype(np.float64)
    p = [t.cpu().numpy().astype(np.float64) for t in parts]
    gap = np.abs(d - sum(p))
    tol = 1.01 * U24 * (np.abs(d) + sum(np.abs(t) for t in p))
    frac = float((gap[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0
    print(f"{what}: dw against the sum of its {len(p)} pieces, largest fraction of 1.01 x 2^-24 x (|dw| + sum |dw_i|) {frac:.3f}")
    assert (gap <= tol).all(), (what, frac)


def chunked(loop, splits):
    """Checks inert, chunked, pieces and flags for one loop.  splits: {cap: the frame runs it must produce}."""
    nb = loop.nb
    eng, pristine = engine("capped"), engine("pristine")
    base = outs(loop.call(pristine))
    base_skip = outs(loop.call(pristine, dskip=True)) if loop.has_dskip else None
    rw, bw = loop.ref()
    check_bound(base[0], rw, bw, f"{loop.name} dw, uncapped")
    for k in (0, nb, nb + 1):  # inert
        eng.set_train_chunk_frames(k)
        assert same(outs(loop.call(eng)), base), (loop.name, "cap", k)
    moved = 0
    for k, runs in splits.items():
        assert sum(b - a for a, b in runs) == nb and all(b - a <= k for a, b in runs)
        eng.set_train_chunk_frames(k)
        got = outs(loop.call(eng))
        assert same(got[1:], base[1:]), (loop.name, "cap", k)  # du / dx and the affine sums keep their bits
        check_bound(got[0], rw, bw, f"{loop.name} dw, cap {k}")
        moved += int(not torch.equal(got[0], base[0]))
        if loop.has_dskip:
            skip = outs(loop.call(eng, dskip=True))
            assert torch.equal(skip[0], got[0]) and same(skip[1:], base_skip[1:]), (loop.name, "cap", k, "dskip")
        assert same(outs(loop.call(eng)), got), (loop.name, "cap", k, "two runs")
        assert torch.equal(loop.call(eng, need_dx=False)[0], got[0]), (loop.name, "cap", k, "need_dx=False")
        if len(runs) < nb:  # at cap 1 the pieces are the single frames, which test_frames of the sibling files cover
            pieces_agree(got[0], [loop.call(pristine, fr=slice(a, b))[0] for a, b in runs], f"{loop.name}, cap {k}")
    print(f"{loop.name}: dw changed bits under {moved} of {len(splits)} caps")  # it need not: ranges of one position chunk add up in double


# ------------------------------------------------------------------ 1. the twelve loops, three frames: 1 + 1 + 1 and 2 + 1
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("family,shape", CASES, ids=case_id)
def test_three_frames(family, shape, kind):
    chunked(loop_of(family, kind, shape, 3), {1: [(0, 1), (1, 2), (2, 3)], 2: [(0, 2), (2, 3)]})


# ------------------------------------------------------------------ 2. five frames: 2 + 2 + 1, gbase advances twice before the short chunk
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("family,shape", FIVE, ids=case_id)
def test_five_frames(family, shape, kind):
    chunked(loop_of(family, kind, shape, 5), {2: [(0, 2), (2, 4), (4, 5)]})


# ------------------------------------------------------------------ 3. the C entries into NaN-filled outputs
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("family,shape", [CASES[0], CASES[4], CASES[7]], ids=case_id)
def test_c_entry_writes_every_output(family, shape, kind):
    loop = loop_of(family, kind, shape, 3)
    eng = engine("capped")
    eng.set_train_chunk_frames(1)
    want = outs(loop.call(eng))
    got = [torch.full_like(t, float("nan")) for t in want]
    assert loop.raw(eng, got[0], got[1], got[2:] if kind == "affine" else None) == 0, eng.lib.pp_last_error(eng.ctx)
    torch.cuda.synchronize()
    assert same(got, want), loop.name


# ------------------------------------------------------------------ 4. the three _bn entries: the context's cap and their own argument
def bn_unit(C, h, w):
    rng = np.random.default_rng(500 + C + h)  # the case of test_bnbatch_gpu.test_unit
    u = rng.standard_normal((3, C, h, w)).astype(np.float32)
    wt = (rng.standard_normal((C, C, 3, 3)) * 0.05).astype(np.float32)
    dz, dskip = rng.standard_normal(u.shape).astype(np.float32), rng.standard_normal(u.shape).astype(np.float32)
    st = folded32(u, rng, C)
    ud, wd, dzd, dsd = (dev(t) for t in (u, wt, dz, dskip))
    std = [dev(t) for t in st]
    want, bounds = BB.unit_bounds(u, wt, *st, dz, dskip=dskip)
    return (lambda eng, k: eng.unit_backward_bn(ud, wd, *std, dzd, dskip=dsd, chunk_frames=k)), (want[0], bounds[0])


def bn_down(cin, cout, hin, win):
    rng = np.random.default_rng(600 + cout + hin)  # the case of test_bnbatch_gpu.test_down
    x = rng.standard_normal((3, cin, hin, win)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3)) * 0.05).astype(np.float32)
    z = BB.D.conv_s2(x, wt).astype(np.float32)
    dy = rng.standard_normal(z.shape).astype(np.float32)
    st = folded32(z, rng, cout)
    xd, wd, zd, dyd = (dev(t) for t in (x, wt, z, dy))
    std = [dev(t) for t in st]
    want, bounds = BB.down_bounds(x, wt, z, *st, dy)
    return (lambda eng, k: eng.down_backward_bn(xd, wd, zd, *std, dyd, chunk_frames=k)), (want[0], bounds[0])


def bn_neck(branch):
    rng = np.random.default_rng(700 + branch)  # the three-frame case of test_bnbatch_gpu.test_neck on this map
    cin, cup, coff, s = BB.N.CIN[branch], BB.N.CUP[branch], BB.N.COFF[branch], 1 << branch
    sl = slice(coff, coff + cup)
    wt = (rng.standard_normal((cin, cup, s, s)) * 0.05).astype(np.float32)
    x = rng.standard_normal((3, cin, H >> branch, W >> branch)).astype(np.float32)
    Z = BB.N.conv_t(x, wt)
    st = folded32(Z, rng, cup)
    y = rng.standard_normal((3, 320, H, W)).astype(np.float32)
    y[:, sl] = np.maximum(BB.aff(Z, st[0], st[1]), 0.0).astype(np.float32)
    y[0, coff, 0, :3] = (0.0, 1.0, 0.0)
    dy = rng.standard_normal(y.shape).astype(np.float32)
    xd, wd, yd, dyd = (dev(t) for t in (x, wt, y, dy))
    std = [dev(t) for t in st]
    want, bounds = BB.branch_backward(x, wt, st[0], st[2], st[3], y[:, sl], dy[:, sl], bounds=True)
    return (lambda eng, k: eng.neck_backward_bn(branch, xd, wd, *std, yd, dyd, chunk_frames=k)), (want[0], bounds[0])


@pytest.mark.parametrize("family,shape", [("unit", (64, 33, 17)), ("unit", (128, 8, 6)), ("unit", (256, 3, 2)), ("down", (64, 64, 32, 24)),
                                          ("down", (64, 128, 17, 9)), ("down", (128, 256, 8, 6)), ("neck", 0), ("neck", 1), ("neck", 2)], ids=case_id)
def test_bn_entries_compose_the_two_caps(family, shape):
    call, bound_w = {"unit": lambda: bn_unit(*shape), "down": lambda: bn_down(*shape), "neck": lambda: bn_neck(shape)}[family]()
    eng, pristine = engine("capped"), engine("pristine")
    what = f"{family}_backward_bn {case_id(shape)}"
    base = call(pristine, 0)
    check_bound(base[0], *bound_w, f"{what} dw, uncapped")
    own = {k: call(pristine, k) for k in (1, 2)}  # the entry's own argument, no context cap

    def ctx_cap(k, own_k=0):
        eng.set_train_chunk_frames(k)
        return call(eng, own_k)

    chunks_agree(ctx_cap, base, bound_w, what + ", context cap")  # du / dx and the sums keep their bits, dw stays inside its bound
    for k in (1, 2):
        assert same(ctx_cap(k), own[k]), (what, "context cap", k, "is not chunk_frames", k)  # every output, dw included
    assert same(ctx_cap(2, 1), own[1]) and same(ctx_cap(1, 2), own[1]), what  # the smaller of the non-zero values
    assert same(ctx_cap(0, 2), own[2]) and same(ctx_cap(5, 2), own[2]) and same(ctx_cap(3), base) and same(ctx_cap(0), base), what


# ------------------------------------------------------------------ 5. the setter
def test_setter():
    loop = unit_loop("fp32", 128, 20, 18, 3)
    eng, pristine = engine("capped"), engine("pristine")
    base = outs(loop.call(pristine))  # a context nobody has set a cap on runs the workspace rule: it starts at 0
    eng.set_train_chunk_frames(0)
    assert same(outs(loop.call(eng)), base)
    eng.set_train_chunk_frames(1)
    capped = outs(loop.call(eng))
    assert not torch.equal(capped[0], base[0])
    with pytest.raises(RuntimeError, match="k must be >= 0"):
        eng.set_train_chunk_frames(-1)
    assert same(outs(loop.call(eng)), capped)  # refused, and the cap of 1 stays in force
    assert eng.lib.pp_set_train_chunk_frames(eng.ctx, -7) != 0 and b"pp_set_train_chunk_frames" in eng.lib.pp_last_error(eng.ctx)
    assert eng.lib.pp_set_train_chunk_frames(None, 1) != 0
    assert same(outs(loop.call(eng)), capped)
    for bad in (1.0, "1", None, True):
        with pytest.raises(ValueError):
            eng.set_train_chunk_frames(bad)
    fresh = ENG(small_cfg(2 * H, 2 * W, 5))
    assert same(outs(loop.call(fresh)), base)
    eng.set_train_chunk_frames(0)
    assert same(outs(loop.call(eng)), base)


# ------------------------------------------------------------------ 6. the autograd surface, two frames in chunks of one
def surface(net, canvas, dy, after=None):
    """One backward of rpn_train on the fixture's canvases, uncapped and at cap 1 -> the capped parameter gradients by name, the
    engine calls the capped run made (after(net) installs the recorders), and the two canvas gradients."""
    eng = net._eng
    runs = []
    try:
        for k in (0, 1):
            eng.set_train_chunk_frames(k)
            seen = after(net) if after and k else None
            net.zero_grad()
            cvg = canvas.clone().requires_grad_()
            net.rpn_train(cvg).backward(dy)
            runs.append(({n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}, cvg.grad.clone(), seen))
    finally:
        eng.set_train_chunk_frames(0)
    (g0, c0, _), (g1, c1, seen) = runs
    assert torch.equal(c0, c1), "the gradient that reaches the canvas depends on the chunking"
    return g1, c1, seen


def rpn_fixture_net():
    """The network of test_rpntrain_gpu.test_fixture_chain."""
    canvas, ws, dy = GR.small_inputs()
    cfg = small_cfg(canvas.shape[2], canvas.shape[3], 2)
    load_pkg("framework.voxel_generator").VoxelGenerator(cfg)
    net = load_pkg("networks.pointpillars8_shared").PointPillars(cfg)
    sd = {k: np.asarray(v, np.float32) for k, v in load_pkg("synth").seeded_state_dict(0).items()}
    for k, w in zip(RR.KEYS, ws):
        assert sd[k].shape == w.shape, k
        sd[k] = w
    net.load_state_dict(sd)
    assert canvas.shape[0] == 2
    return net, dev(canvas), dev(dy)


def test_surface_fp32():
    """test_rpntrain_gpu.test_fixture_chain with every backward of the chain in chunks of one frame: its bar, 4 x ref32_dev x max |g64|."""
    load_pkg().install()
    g = golden("rpntrain_small")
    net, cv, dy = rpn_fixture_net()
    net.train(scope="rpn")
    grads, dcanvas, _ = surface(net, cv, dy)
    for i, k in enumerate(RR.KEYS):
        check_grad(grads[k].reshape(-1)[::GR.DW_STRIDE], g[f"dw_{i}"], float(g[f"ref32_dev_dw_{i}"]), float(g[f"dw_{i}_max"]), f"cap 1, golden dw {k}")
    check_grad(dcanvas.reshape(-1)[::GR.DX_STRIDE], g["dcanvas"], float(g["ref32_dev_dcanvas"]), float(g["dcanvas_max"]), "cap 1, golden dcanvas")


def test_surface_bf16x3(monkeypatch):
    """The same chain with grad_precision="bf16x3", grad_stages="rpn": every weight gradient inside the a-priori bound of its own call,
    evaluated from the tensors the call saw, which is what the surface tests of test_mixedtrain_gpu / test_mixedstage_gpu assert."""
    load_pkg().install()
    net, cv, dy = rpn_fixture_net()
    net.train(scope="rpn", grad_precision="bf16x3", grad_stages="rpn")

    def record(net):
        eng, seen = net._eng, []
        unit, down, neck = eng.unit_backward, eng.down_backward, eng.neck_backward

        def rec_unit(u, w, dy, **kw):
            out = unit(u, w, dy, **kw)
            seen.append(("unit", w, (u, dy), kw.get("grad_precision"), out[0]))
            return out

        def rec_down(x, w, z, dy, **kw):
            out = down(x, w, z, dy, **kw)
            seen.append(("down", w, (x, z, dy), kw.get("grad_precision"), out[0]))
            return out

        def rec_neck(branch, x, w, y, dy, **kw):
            out = neck(branch, x, w, y, dy, **kw)
            seen.append(("neck", w, (branch, x, y, dy), kw.get("grad_precision"), out[0]))
            return out

        monkeypatch.setattr(eng, "unit_backward", rec_unit)
        monkeypatch.setattr(eng, "down_backward", rec_down)
        monkeypatch.setattr(eng, "neck_backward", rec_neck)
        return seen

    grads, _, seen = surface(net, cv, dy, after=record)
    assert len(seen) == 19 and all(c[3] == "bf16x3" for c in seen)
    params = dict(net.named_parameters())
    by_weight = {c[1].data_ptr(): c for c in seen}
    n64 = lambda *ts: [t.detach().cpu().numpy() for t in ts]  # noqa: E731
    for k in RR.KEYS:
        family, _, args, _, dw = by_weight[params[k].data_ptr()]
        assert torch.equal(dw, grads[k]), k  # what the call returned is what autograd delivered
        if family == "unit":
            rw, _, bw, _, ties = M.grad_bounds_mixed(*n64(args[0], params[k], args[1]), "bf16x3")
        elif family == "down":
            rw, _, bw, _, ties = S.down_grad_bounds_mixed(*n64(args[0], params[k], args[1], args[2]), "bf16x3")
        else:
            sl = S.branch_slice(args[0])
            rw, _, bw, _ = S.neck_grad_bounds_mixed(*n64(args[1], params[k], args[2][:, sl], args[3][:, sl]), "bf16x3")
            ties = np.zeros(1, bool)
        assert ties.sum() <= 1e-3 * ties.size, k
        check_bound(dw, rw, bw, f"cap 1, bf16x3 autograd dw {k}")


def test_surface_frozen_batchnorm():
    """test_bntrain_gpu.test_fixture_chain (the BatchNorm network, bn_stats="frozen") in chunks of one frame: its bar."""
    load_pkg().install()
    g = golden("bntrain_small")
    canvas, ws, bn, dy = GB.small_inputs()
    assert canvas.shape[0] == 2
    net, _ = bn_net(canvas.shape[2], canvas.shape[3], max_batch=2)
    sd = bn_sd()
    for k, w in zip(A.LAYER_KEYS, ws):
        assert sd[k].shape == w.shape, k
        sd[k] = w
    for pfx, t in zip(A.BN_PREFIXES, bn):
        sd.update({f"{pfx}.{s}": v for s, v in zip(ENG.BN_FIELDS, t)})
    net.load_state_dict(sd)
    net.train(scope="rpn", bn_stats="frozen")
    names = [k for k, _ in net.named_parameters()]
    assert names[:57] == [str(k) for k in g["param_names"]]
    grads, dcanvas, _ = surface(net, dev(canvas), dev(dy))
    for i, k in enumerate(names[:57]):
        got = grads[k].reshape(-1)
        check_grad(got[::GB.DW_STRIDE] if grads[k].dim() == 4 else got, g[f"g_{i}"], float(g[f"ref32_dev_g_{i}"]), float(g[f"g_{i}_max"]),
                   f"cap 1, golden {k}")
    check_grad(dcanvas.reshape(-1)[::GB.DX_STRIDE], g["dcanvas"], float(g["ref32_dev_dcanvas"]), float(g["dcanvas_max"]), "cap 1, golden dcanvas")
