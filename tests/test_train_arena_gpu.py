"""GPU: the training entries on arenas (tests/arena.py).  Every pointer argument of a call sits in an allocation of its own with no
contractual slack (the header grants these arguments none), surrounded by 64 KB or a frame of one of the fills "zeros", "nan" and
"poison"; outputs start pre-filled; a tensor that an entry updates in place keeps its contents.  Each entry is called through eng.lib
with ctypes, in the argument order tests/test_trainargs_gpu.py tabulates.  Per case:
  (a) the zero-fill run is held to the float64 reference under the bar of the family's own GPU test, with that test's functions: no new
      tolerance;
  (b) the "nan" and "poison" runs reproduce the zero-fill run's outputs bit for bit (the entries are documented as deterministic with no
      atomics: equality is the contract), dscale / dshift (fp64) included;
  (c) arena.untouched holds for every argument, inputs included, after every run;
  (d) the "nan" run pre-fills its outputs with the byte 0x5A, the other two with 0xA5.  An element the kernel never stored would differ
      between the runs, so (b) already fails on it: no element is excluded and no cap is needed.  Do NOT "fix" a failure of (b) by
      pre-filling the runs alike;
  (e) one further run (poison fill) with every pointer the header does not constrain at an address % 16 == 4; w (16 bytes), the fp64 sums
      and statistics (8), dir / ddir (8, in pp_head_backward too: the tensor is pp_target_loss_grad's) and the PFN voxels (16) keep exactly
      the alignment the header demands and no more.  It must return 0 and reproduce (b)'s bits.

Families (KIND: mode 0 is the fp32 entry itself, modes 1 bf16x3 and 2 bf16 the _mp twin, asserted through the matching _path entry to
run in the mode asked for; form "in" runs on an InstanceNorm engine, "affine" / "bn" on a norm="batch" engine):
  unit   pp_unit_backward{,_affine,_bn}{,_mp}, all forms x modes, (C, h, w, nb) = (64, 5, 7, 2), (128, 3, 6, 3), (256, 2, 20, 1),
         (256, 1, 7, 2); each with dskip and du, without dskip, and with du NULL (the affine / bn forms then without dscale / dshift, as
         the entry demands; dw keeps its bits): (a) - (e).
  down   pp_down_backward{,_affine,_bn}{,_mp}, all forms x modes, (cin, cout, hin, win, nb) = (64, 64, 5, 7, 2), (128, 256, 2, 3, 2),
         (64, 128, 1, 4, 1); with and without dx: (a) - (e).
  neck   pp_neck_backward{,_affine,_bn}{,_mp}, all forms x modes x branches on the level-0 maps (H, W, nb) = (4, 4, 2) and (20, 36, 2);
         y / dy are the full 320-channel tensors, and a further run whose y and dy hold the poison words in the other branches' channels
         must give the bits of the run where dy holds zeros there: (a) - (e).
  chunks one case per family with nb = 3 in chunks of two frames (chunk_frames of the _bn entries, pp_set_train_chunk_frames for the
         others), all forms x modes: unit (64, 5, 7), down (64, 64, 5, 7), neck branch 1 on (4, 4): (a) - (e).
  two plane segments (SEG_ELEMS = 16384): unit (64, 129, 128, 1) and down (64, 64, 260, 254, 1), forms "in" and "bn", fp32 and mode 2:
         (a) - (d).  (a) is held everywhere: the float64 bounds of these planes take 2 to 5 s on the host, so no case skips it for host
         time; (e) is left to the small shapes.
  head   pp_target_loss_grad and pp_head_backward on the 8 x 6 map of test_headtrain_gpu.py with 1 and 2 frames, and on a 7 x 5 map
         (grid 14 x 10, A = 35 na: with the configuration's na an anchor count that is no multiple of 4 exists, so vec == 0 is reached
         through A % 4 as well as through a pointer): (a) - (e).  Loss gradient: 4 x ref32_dev x max |g64| against headtrain_ref.loss_grad;
         head backward: the summation bound of test_headtrain_gpu.check_backward.
  pfn    pp_pfn_train_forward, pp_pfn_backward, pp_scatter_backward on the two frames of train_common.two_frames cut to 40 pillars each,
         npts holding 1 and T: (a) - (e), at the bars of test_pfntrain_gpu.test_large_batch_of_pillars (the restatement at the GPU's own
         selection, which must maximise to within 1e-5); the scatter's backward is a gather and is compared exactly.
  optim  pp_grad_norm, pp_scale_grads, pp_adam_step over eight tensors (GROUP - 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 CHUNK + 7, 1, 3, 5
         elements), every tensor in its own arena, p / exp_avg / exp_avg_sq and the scaled gradients in place: (a) - (e) at the bars of
         test_optim_gpu (norm 2^-23 relative, the scaled gradient numpy's fp32 product, the step test_optim_gpu.bars).
History: for unit, down and neck, fp32 and mode 2, forms "in" and "bn": on one engine a call of a larger, different geometry whose dy (and
u / x under "bn") holds the poison words leaves +-2^40 across the padded planes, the statistics and the dw partials; the small call
behind it, and the same call once more, must give the bits of that call on an engine that has made no other call."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import golden, load_pkg
import arena as A
import blocktrain_ref as B
import headtrain_ref as RH
import mixedbn_ref as R
import mixedstage_ref as S
import mixedtrain_ref as M
import optim_ref as RO
import pfntrain_ref as RP
from train_common import GX, GY, check_bound, dev, random_case, seeded_sd, small_cfg, two_frames

pytestmark = pytest.mark.gpu
ENG = load_pkg("engine").Engine
KIND = ("fp32", "bf16x3", "bf16")
FORMS = ("in", "affine", "bn")
SUFFIX = {"in": "", "affine": "_affine", "bn": "_bn"}
UNIT_SHAPES = [(64, 5, 7, 2), (128, 3, 6, 3), (256, 2, 20, 1), (256, 1, 7, 2)]
DOWN_SHAPES = [(64, 64, 5, 7, 2), (128, 256, 2, 3, 2), (64, 128, 1, 4, 1)]
NECK_MAPS = [(4, 4, 2), (20, 36, 2)]
UNIT_TWO_SEGMENTS, DOWN_TWO_SEGMENTS = (64, 129, 128, 1), S.DOWN_SHAPES[-1]
ODD_OFFSET = {4: 260, 8: 264, 16: 272}  # an address with exactly that alignment, in a 512-byte block
_ENGINES = {}


def engine(gx=24, gy=16, max_batch=3, norm="instance", fresh=False):
    """An engine without weights (the backwards are stateless).  fresh: one nobody else holds."""
    load_pkg().install()
    if fresh:
        return ENG(small_cfg(gx, gy, max_batch), norm=norm)
    key = (gx, gy, max_batch, norm)
    if key not in _ENGINES:
        _ENGINES[key] = ENG(small_cfg(gx, gy, max_batch), norm=norm)
    return _ENGINES[key]


def norm_kind(form):
    return "instance" if form == "in" else "batch"


# ------------------------------------------------------------------ arguments on arenas
class Arg:
    """A pointer argument: role "in" (value: a tensor or an array, put on the device by run), "io" (updated in place) or "out" (value:
    (shape, dtype)); align: what the header demands of the pointer, kept and not exceeded by the run of (e)."""

    def __init__(self, name, role, value, align=4):
        self.name, self.role, self.value, self.align = name, role, value, align


def In(name, t, align=4):
    return None if t is None else Arg(name, "in", t, align)


def IO(name, t):
    return Arg(name, "io", t)


def Out(name, shape, dtype=torch.float32, align=4):
    return Arg(name, "out", (tuple(shape), dtype), align)


class Ptrs:
    """A HOST array of device pointers, one arena per entry (None: a null entry)."""

    def __init__(self, args):
        self.args = list(args)


def run(eng, entry, args, fill, odd=False):
    """Calls eng.lib.<entry>(ctx, *args) with every Arg in an arena of fill `fill` -> {name: a copy of the tensor} for the "out" and "io"
    arguments.  Asserts the return code and (c)."""
    arenas = []

    def placed(a):
        if a is None:
            return None
        off = ODD_OFFSET[a.align] if odd else A.OFFSET
        if a.role == "out":
            ar = A.place_out(a.value[0], a.value[1], fill="5a" if fill == "nan" else "a5", offset=off)
        else:
            ar = A.place(a.value.cuda() if isinstance(a.value, torch.Tensor) else dev(a.value), 0, 0, fill, offset=off, inplace=a.role == "io")
        assert ar.ptr % 16 == (a.align % 16 if odd else 0)
        arenas.append((a, ar))
        return ar.ptr

    raw = []
    for a in args:
        if isinstance(a, Ptrs):
            raw.append((ctypes.c_void_p * max(1, len(a.args)))(*[placed(x) for x in a.args]))
        elif isinstance(a, Arg):
            raw.append(placed(a))
        else:
            raw.append(a)
    rc = getattr(eng.lib, entry)(eng.ctx, *raw)
    torch.cuda.synchronize()
    assert rc == 0, (entry, fill, odd, rc, eng.lib.pp_last_error(eng.ctx).decode())
    for a, ar in arenas:
        assert A.untouched(ar), f"{entry}, fill {fill}{', odd pointers' if odd else ''}: the call changed memory outside {a.name}" + \
            ("" if a.role != "in" else " or the input itself")
    return {a.name: ar.t.clone() for a, ar in arenas if a.role != "in"}


def bits(t):
    return t.view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_same(got, want, what):
    assert got.keys() == want.keys(), what
    for k in want:
        diff = int((bits(got[k]) != bits(want[k])).sum())
        assert diff == 0, f"{what}: {k} differs in {diff} of {want[k].numel()} elements"


def held(eng, entry, args, what, odd=True):
    """(b), (c), (d) and, with odd, (e) -> the zero-fill run's outputs."""
    runs = {fill: run(eng, entry, args, fill) for fill in A.FILLS}
    for fill in ("nan", "poison"):
        assert_same(runs[fill], runs["zeros"], f"{what}: fill {fill} against zeros")
    if odd:
        assert_same(run(eng, entry, args, "poison", odd=True), runs["zeros"], f"{what}: pointers at % 16 == 4")
    return runs["zeros"]


def poison_like(shape):
    """float32 +-2^40, element i positive when i is even: arena's poison words as a tensor."""
    n = int(np.prod(shape))
    return np.where(np.arange(n) % 2 == 0, np.float32(2.0 ** 40), np.float32(-2.0 ** 40)).astype(np.float32).reshape(shape)


# ------------------------------------------------------------------ the backward families: inputs, references, calls
@functools.lru_cache(maxsize=None)
def inputs(fam, shape, form):
    """The case makers of the sibling files.  unit: u, w, norm, dz, dskip; down: x, w, z, norm, dy; neck: xs, ws, norms, y, dy (norm: () under
    form "in", (scale, shift) under "affine", (scale, shift, mean, var) under "bn")."""
    rform = {"affine": "affine", "bn": "batch"}.get(form)
    if fam == "unit":
        C, h, w, nb = shape
        if form == "in":
            u, wt, dz, dskip = random_case(C, h, w, nb, 100 + C + h)  # asserts that no |xhat| < 1e-4
            return u, wt, (), dz, dskip
        return R.unit_case(C, h, w, nb, rform)
    if fam == "down":
        if form == "in":
            x, wt, z, dy = S.down_case(*shape)
            return x, wt, z, (), dy
        return R.down_case(*shape, rform)
    if form == "in":
        xs, ws, y, dy = S.neck_case(*shape)
        return xs, ws, [()] * 3, y, dy
    return R.neck_case(*shape, rform)


@functools.lru_cache(maxsize=None)
def terms(fam, shape, form, branch=None):
    """The mode-independent part of the bounds."""
    c = inputs(fam, shape, form)
    if fam == "unit":
        return None if form == "in" else R.unit_terms(c[0], c[1], c[2], c[3])
    if fam == "down":
        if form == "in":
            t = S.down_terms(c[0], c[1], c[2], c[4])
            assert not t["ties"].any()
            return t
        return R.down_terms(*c)
    xs, ws, norms, y, dy = c
    sl = S.branch_slice(branch)
    if form == "in":
        return S.neck_terms(xs[branch], ws[branch], y[:, sl], dy[:, sl])
    return R.neck_terms(xs[branch], ws[branch], norms[branch], y[:, sl], dy[:, sl])


def reference(fam, shape, form, mode, dskip=True, branch=None):
    """-> (dw, dx, [dscale, dshift]) in float64 and their element-wise a-priori bounds, from the functions the family's GPU test uses."""
    c, kind = inputs(fam, shape, form), KIND[mode]
    if fam == "unit":
        u, wt, norm, dz, ds = c
        ds = ds if dskip else None
        if form == "in":
            rw, ru, bw, bu, ties = B.grad_bounds(u, wt, dz, dskip=ds) if mode == 0 else M.grad_bounds_mixed(u, wt, dz, kind, dskip=ds)
            assert not ties.any()
            return (rw, ru), (bw, bu)
        return R.unit_bounds_mixed(u, wt, norm, dz, kind, dskip=ds, terms=terms(fam, shape, form))
    t = terms(fam, shape, form, branch)
    if form != "in":
        return R.stage_bounds_mixed(t, kind)
    if fam == "down":
        rw, rx, bw, bx, _ = S.down_grad_bounds_mixed(*c[:3], c[4], kind, terms=t)  # "fp32": downtrain_ref.grad_bounds itself
    else:
        rw, rx, bw, bx = S.neck_grad_bounds_mixed(None, None, None, None, kind, terms=t)  # "fp32": necktrain_ref.grad_bounds itself
    return (rw, rx), (bw, bx)


def call_of(fam, shape, form, mode, dskip=True, dx=True, branch=None, chunk_frames=0, dy=None, lead=None, y=None):
    """-> (entry, the integers of the shape, the arguments behind the context).  dy / lead / y: other contents for dy, for u (unit) or x,
    and for the upsampler's y."""
    c = inputs(fam, shape, form)
    nb = shape[-1]
    if fam == "unit":
        u, wt, norm, dz, ds = c
        ints, C = list(shape[:3]), shape[0]
        pre, post = [In("u", u if lead is None else lead), In("w", wt, 16)], [In("dy", dz if dy is None else dy), In("dskip", ds if dskip else None)]
        outs = [Out("dw", wt.shape), Out("du", u.shape) if dx else None]
        sums = dx  # the sums are sums over the dgrad product
    elif fam == "down":
        x, wt, z, norm, dyc = c
        ints, C = list(shape[:4]), shape[1]
        pre, post = [In("x", x if lead is None else lead), In("w", wt, 16), In("z", z)], [In("dy", dyc if dy is None else dy)]
        outs = [Out("dw", wt.shape), Out("dx", x.shape) if dx else None]
        sums = True
    else:
        xs, ws, norms, yc, dyc = c
        ints, C, norm = [branch], ws[branch].shape[1], norms[branch]
        pre, post = [In("x", xs[branch] if lead is None else lead), In("w", ws[branch], 16)], [In("y", yc if y is None else y), In("dy", dyc if dy is None else dy)]
        outs = [Out("dw", ws[branch].shape), Out("dx", xs[branch].shape) if dx else None]
        sums = True
    if form != "in":
        outs += [Out(n, (C,), torch.float64, 8) if sums else None for n in ("dscale", "dshift")]
    names = ("scale", "shift", "mean", "var")
    args = ([mode] if mode else []) + ints + pre + [In(n, t) for n, t in zip(names, norm)] + post + [nb] + outs + ([chunk_frames] if form == "bn" else []) + [None]
    return f"pp_{fam}_backward{SUFFIX[form]}{'_mp' if mode else ''}", ints, args


def assert_path(eng, fam, form, mode, ints):
    """The mode asked for is the mode that runs: otherwise the arena would cover the fp32 fallback."""
    if mode:
        query = f"pp_{fam}_backward{'' if form == 'in' else '_bn'}_path"
        assert getattr(eng.lib, query)(eng.ctx, mode, *ints) == mode, (query, mode, ints)


def check(got, want, bounds, what):
    """(a)"""
    for name, w, b in zip(("dw", "dx", "dscale", "dshift"), want, bounds):
        key = "du" if name == "dx" and "du" in got else name
        if key in got:
            check_bound(got[key], w, b, f"{what} {key}")


def case(fam, shape, form, mode, eng=None, odd=True, ref=True, **kw):
    """One call held to (a) - (e) -> the zero-fill run's outputs."""
    eng = engine(norm=norm_kind(form)) if eng is None else eng
    entry, ints, args = call_of(fam, shape, form, mode, **kw)
    assert_path(eng, fam, form, mode, ints)
    what = f"{entry} {shape} {KIND[mode]} {({k: v for k, v in kw.items() if not isinstance(v, np.ndarray)})}"
    got = held(eng, entry, args, what, odd=odd)
    if ref:
        check(got, *reference(fam, shape, form, mode, dskip=kw.get("dskip", True), branch=kw.get("branch")), what)
    return got


def ident(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else KIND[v] if isinstance(v, int) else str(v)


# ------------------------------------------------------------------ 1. units
@pytest.mark.parametrize("mode", (0, 1, 2), ids=ident)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", UNIT_SHAPES, ids=ident)
def test_unit(shape, form, mode):
    full = case("unit", shape, form, mode)
    case("unit", shape, form, mode, dskip=False)
    only_dw = case("unit", shape, form, mode, dx=False)
    assert set(only_dw) == {"dw"}
    assert_same(only_dw, {"dw": full["dw"]}, f"unit {shape} {form} {KIND[mode]}: dw with du NULL")


# ------------------------------------------------------------------ 2. strided stages
@pytest.mark.parametrize("mode", (0, 1, 2), ids=ident)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", DOWN_SHAPES, ids=ident)
def test_down(shape, form, mode):
    full = case("down", shape, form, mode)
    no_dx = case("down", shape, form, mode, dx=False)
    assert "dx" not in no_dx
    assert_same(no_dx, {k: full[k] for k in no_dx}, f"down {shape} {form} {KIND[mode]}: dx NULL")  # the header: dw is the same bits


# ------------------------------------------------------------------ 3. upsamplers
@pytest.mark.parametrize("mode", (0, 1, 2), ids=ident)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", NECK_MAPS, ids=ident)
def test_neck(shape, form, mode):
    H, W, nb = shape
    eng = engine(2 * H, 2 * W, 3, norm_kind(form))
    y, dy = inputs("neck", shape, form)[3:]
    for b in range(3):
        sl = S.branch_slice(b)
        zeroed, poisoned, ypoisoned = np.zeros_like(dy), poison_like(dy.shape), poison_like(y.shape)
        zeroed[:, sl] = poisoned[:, sl] = dy[:, sl]
        ypoisoned[:, sl] = y[:, sl]
        got = case("neck", shape, form, mode, eng=eng, branch=b, dy=zeroed)
        entry, _, args = call_of("neck", shape, form, mode, branch=b, dy=poisoned, y=ypoisoned)
        assert_same(run(eng, entry, args, "poison"), got, f"{entry} {shape} branch {b}: the other branches' channels of y and dy hold +-2^40")
        no_dx = case("neck", shape, form, mode, eng=eng, branch=b, dx=False, odd=False)
        assert_same(no_dx, {k: got[k] for k in no_dx}, f"{entry} {shape} branch {b}: dx NULL")


# ------------------------------------------------------------------ 4. three frames in chunks of two
CHUNKED = [("unit", (64, 5, 7, 3), None), ("down", (64, 64, 5, 7, 3), None), ("neck", (4, 4, 3), 1)]


@pytest.mark.parametrize("mode", (0, 1, 2), ids=ident)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("fam,shape,branch", CHUNKED, ids=[c[0] for c in CHUNKED])
def test_frame_chunks(fam, shape, branch, form, mode):
    eng = engine(*((2 * shape[0], 2 * shape[1]) if fam == "neck" else (24, 16)), 3, norm_kind(form))
    kw = {} if branch is None else {"branch": branch}
    try:
        if form == "bn":
            kw["chunk_frames"] = 2
        else:
            eng.set_train_chunk_frames(2)
        case(fam, shape, form, mode, eng=eng, **kw)
    finally:
        eng.set_train_chunk_frames(0)


# ------------------------------------------------------------------ 5. two plane segments
@pytest.mark.parametrize("mode", (0, 2), ids=ident)
@pytest.mark.parametrize("form", ("in", "bn"))
@pytest.mark.parametrize("fam,shape", [("unit", UNIT_TWO_SEGMENTS), ("down", DOWN_TWO_SEGMENTS)], ids=("unit", "down"))
def test_two_plane_segments(fam, shape, form, mode):
    """(a) - (d): the float64 bounds of these planes take 2 to 5 s on the host per form (shared by the two modes), so (a) is held."""
    positions = shape[1] * shape[2] if fam == "unit" else ((shape[2] + 1) // 2) * ((shape[3] + 1) // 2)
    assert positions > 16384
    case(fam, shape, form, mode, odd=False)


# ------------------------------------------------------------------ 6. independence of history
DIRTY = {"unit": (64, 12, 11, 3), "down": (64, 128, 12, 11, 3)}
SMALL = {"unit": UNIT_SHAPES[0], "down": DOWN_SHAPES[0], "neck": (20, 36, 2)}


def dirtying(eng, fam, shape, form, mode, branch=None):
    """A call whose dy (and u / x under "bn") holds the poison words: return code 0, outputs not judged."""
    c = inputs(fam, shape, form)
    lead = None if form == "in" else poison_like((c[0] if fam != "neck" else c[0][branch]).shape)
    dy = poison_like((c[3] if fam == "unit" else c[4]).shape)
    entry, _, args = call_of(fam, shape, form, mode, branch=branch, dy=dy, lead=lead)
    run(eng, entry, args, "zeros")


@pytest.mark.parametrize("mode", (0, 2), ids=ident)
@pytest.mark.parametrize("form", ("in", "bn"))
@pytest.mark.parametrize("fam,b", [("unit", None), ("down", None), ("neck", 0), ("neck", 1), ("neck", 2)], ids=("unit", "down", "neck0", "neck1", "neck2"))
def test_history(fam, b, form, mode):
    shape = SMALL[fam]
    geom = (2 * shape[0], 2 * shape[1]) if fam == "neck" else (24, 16)
    used, fresh = (engine(*geom, 3, norm_kind(form), fresh=True) for _ in range(2))
    kw = {} if b is None else {"branch": b}
    entry, ints, args = call_of(fam, shape, form, mode, **kw)
    assert_path(used, fam, form, mode, ints)
    want = run(fresh, entry, args, "zeros")
    for f in ("unit", "down"):  # the larger shapes of another geometry: 12 x 11 maps, three frames, other channel counts
        dirtying(used, f, DIRTY[f], form, mode)
    if fam == "neck":  # the upsamplers' map is the engine's: three frames of every branch
        for other in range(3):
            dirtying(used, "neck", shape[:2] + (3,), form, mode, branch=other)
    assert_same(run(used, entry, args, "zeros"), want, f"{entry} {shape} {kw} behind poisoned calls of another geometry")
    assert_same(run(used, entry, args, "zeros"), want, f"{entry} {shape} {kw} behind itself")


# ------------------------------------------------------------------ 7. loss gradient and head backward
@functools.lru_cache(maxsize=None)
def head_engine(gx, gy):
    """An engine with the fixture's head weights over the seeded backbone (pp_head_backward's dx reads the committed head)."""
    import sys
    from conftest import GOLDEN
    sys.path.insert(0, GOLDEN)
    from make_headtrain_goldens import small_inputs
    load_pkg().install()
    eng = ENG(small_cfg(gx, gy, 2))
    x, sd, labels, tgt, dirt = small_inputs()
    full = seeded_sd()
    full.update({k: np.asarray(v, np.float32) for k, v in sd.items()})
    eng.load_state_dict(full)
    return eng, RH.natural_weights(sd)[0], (x, labels, tgt, dirt)


def head_case(gx, gy, nb):
    eng, Wn, (x, labels, tgt, dirt) = head_engine(gx, gy)
    H, W, A_ = eng.H, eng.W, eng.A
    if (gx, gy) == (16, 12):
        g = golden("headtrain_small")
        assert x.shape == (2, 320, 8, 6) and labels.shape == (2, A_)
        cls, box, dr = (np.asarray(g[k], np.float32) for k in ("logits_cls", "logits_box", "logits_dir"))
        t = [a[:nb] for a in (x, cls.reshape(2, A_), box.reshape(2, A_, 7), dr.reshape(2, A_, 2), labels.reshape(2, A_), tgt.reshape(2, A_, 7),
                              dirt.reshape(2, A_))]
    else:
        rng = np.random.default_rng(70 + gx)
        u = rng.random((nb, A_))
        lab = np.where(u < 1 / 7, 1, np.where(u < 0.75, 0, -1)).astype(np.int32)
        t = [np.maximum(rng.standard_normal((nb, 320, H, W)), 0).astype(np.float32), rng.standard_normal((nb, A_)).astype(np.float32),
             (rng.standard_normal((nb, A_, 7)) * 0.5).astype(np.float32), rng.standard_normal((nb, A_, 2)).astype(np.float32), lab,
             (rng.standard_normal((nb, A_, 7)) * 0.4).astype(np.float32), (rng.random((nb, A_)) < 0.5).astype(np.int32)]
    kinds = (np.float32, np.float32, np.float32, np.float32, np.int32, np.float32, np.int32)
    return eng, Wn, [np.ascontiguousarray(a, k) for a, k in zip(t, kinds)]


@pytest.mark.parametrize("gx,gy,nb", [(16, 12, 1), (16, 12, 2), (14, 10, 2)], ids=("8x6x1", "8x6x2", "7x5x2"))
def test_head(gx, gy, nb):
    eng, Wn, (x, cls, box, dr, lab, tgt, dirt) = head_case(gx, gy, nb)
    na, A_, P = eng.num_anchor_per_loc, eng.A, eng.H * eng.W
    assert A_ == na * P and ((gx, gy) == (16, 12) or A_ % 4 != 0)
    g = golden("headtrain_small")
    args = [In("cls", cls), In("box", box), In("dir", dr, 8), In("labels", lab), In("bbox_targets", tgt), In("dir_targets", dirt), nb, nb, 1.0,
            Out("dcls", (nb, A_, 1)), Out("dbox", (nb, A_, 7)), Out("ddir", (nb, A_, 2), align=8), None]
    got = held(eng, "pp_target_loss_grad", args, f"pp_target_loss_grad {eng.H}x{eng.W}x{nb}")
    want = RH.loss_grad(cls, box, dr, lab, tgt, dirt)
    for n, w in zip(("dcls", "dbox", "ddir"), want):
        a = got[n].cpu().numpy().astype(np.float64).reshape(w.shape)
        bar = 4.0 * float(g["ref32_dev_" + n]) * np.abs(w).max()
        err = np.abs(a - w).max()
        print(f"{n}: max err {err:.3e}, bar {bar:.3e}")
        assert err <= bar, n
        a = a.reshape(nb, A_, -1)
        assert not a[lab == -1].any() and (n == "dcls" or not a[lab <= 0].any())
    dY = [w.astype(np.float32).reshape(s) for w, s in zip(want, ((nb, A_, 1), (nb, A_, 7), (nb, A_, 2)))]
    outs = [Out("dw_cls", (na, 320)), Out("dw_box", (7 * na, 320)), Out("dw_dir", (2 * na, 320)), Out("db_cls", (na,)), Out("db_box", (7 * na,)),
            Out("db_dir", (2 * na,))]
    args = [In("rpn_out", x), In("dcls", dY[0]), In("dbox", dY[1]), In("ddir", dY[2], 8), nb] + outs + [Out("dx", x.shape), None]
    got = held(eng, "pp_head_backward", args, f"pp_head_backward {eng.H}x{eng.W}x{nb}")
    dW, db, dx, (aW, ab, ax) = RH.head_backward(x, *dY, Wn, na, bounds=True)
    gW = np.concatenate([got[k].cpu().numpy() for k in ("dw_cls", "dw_box", "dw_dir")]).astype(np.float64)
    gb = np.concatenate([got[k].cpu().numpy() for k in ("db_cls", "db_box", "db_dir")]).astype(np.float64)
    fr = {"dW": float((np.abs(gW - dW) / RH.sum_bound(nb * P, aW, dW)).max()), "db": float((np.abs(gb - db) / RH.sum_bound(nb * P, ab, db)).max()),
          "dX": float((np.abs(got["dx"].cpu().numpy().astype(np.float64) - dx) / RH.sum_bound(10 * na, ax, dx)).max())}
    print(f"largest fraction of the summation bound {fr}")
    assert max(fr.values()) <= 1.0, fr
    no_dx = held(eng, "pp_head_backward", args[:-2] + [None, None], "pp_head_backward, dx NULL", odd=False)
    assert_same(no_dx, {k: got[k] for k in no_dx}, "pp_head_backward: dx NULL")


# ------------------------------------------------------------------ 8. pillar feature net and scatter
def test_pfn_and_scatter():
    from test_pfntrain_gpu import check as within, frames_of
    load_pkg().install()
    eng = ENG(small_cfg(GX, GY, 2))
    T = eng.T
    frames = [tuple(t[:40].contiguous() for t in f) for f in frames_of(two_frames(eng))]
    v, c, n = (torch.cat([f[i] for f in frames]) for i in range(3))
    n[0], n[1] = 1, T
    P = v.shape[0]
    assert P == 80 and 1 in n.tolist() and T in n.tolist()
    sd = seeded_sd()
    w, gamma, beta = (np.ascontiguousarray(sd[k], np.float32) for k in ENG.PFN_KEYS)
    w = w.reshape(64, 9)
    pillars = [In("voxels", v, 16), In("coors", c), In("npts", n), In("num_pillars", eng.num_tensor(P))]
    args = pillars + [In("w", w), In("gamma", gamma), In("beta", beta), Out("feat", (P, 64)), Out("arg", (P, 64), torch.uint8),
                      Out("stats", (218,), torch.float64, 8), None]
    fw = held(eng, "pp_pfn_train_forward", args, "pp_pfn_train_forward")
    g = golden("pfntrain_small")
    vs, off = eng.voxel_size, eng.offset
    f = RP.features(v.cpu().numpy(), c.cpu().numpy(), n.cpu().numpy(), vs[0], vs[1], vs[0] / np.float32(2) + off[0], vs[1] / np.float32(2) + off[1])
    fwd = RP.forward(f, w, gamma, beta)
    ga, gf = fw["arg"].cpu().numpy(), fw["feat"].cpu().numpy()
    assert RP.maximiser_slack(fwd["y"], ga).max() <= 1e-5
    ok = [within(fw["feat"], fwd["feat"], float(g["ref32_dev_feat_a"]), "feat"), within(fw["stats"][:64], fwd["mean"], float(g["ref32_dev_mean_a"]), "mean"),
          within(fw["stats"][64:128], fwd["var"], float(g["ref32_dev_var_a"]), "var")]
    assert all(ok), ok
    # the scatter's backward, frame by frame: a gather, compared exactly
    rng = np.random.default_rng(12)
    dfeat = []
    for i, (_, ci, _) in enumerate(frames):
        dcanvas = dev(rng.standard_normal((1, 64, GX, GY)).astype(np.float32))
        got = held(eng, "pp_scatter_backward", [In("dcanvas", dcanvas), In("coors", ci), In("num_pillars", eng.num_tensor(40)), Out("dfeat", (40, 64)), None],
                   f"pp_scatter_backward, frame {i}")["dfeat"]
        idx = ci[:, 0].long() * GY + ci[:, 1].long()
        assert torch.equal(got, dcanvas.reshape(64, -1)[:, idx].t().contiguous())
        dfeat.append(got)
    dfeat = torch.cat(dfeat)
    args = pillars + [In("w", w), In("gamma", gamma), In("stats", fw["stats"], 8), In("feat", fw["feat"]), In("arg", fw["arg"]), In("dfeat", dfeat),
                      Out("dw", (64, 9)), Out("dgamma", (64,)), Out("dbeta", (64,)), None]
    bw = held(eng, "pp_pfn_backward", args, "pp_pfn_backward")
    want = RP.backward(f, w, gamma, dict(fwd, feat=gf), dfeat.cpu().numpy(), arg=ga)
    ok = [within(bw[k], w64, float(g[f"ref32_dev_{k}_a"]), k) for k, w64 in zip(("dw", "dgamma", "dbeta"), want)]
    assert all(ok), ok


# ------------------------------------------------------------------ 9. optimizer
def test_optimizer():
    from test_optim_gpu import CHUNK, GROUP, LR, bars
    eng = engine(24, 16, 1)
    lens = [GROUP - 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7, 1, 3, 5]
    rng = np.random.default_rng(5)
    entries = [dict(RO.values(rng, k), kind="plain") for k in lens]
    count = len(lens)
    clens = (ctypes.c_int64 * count)(*lens)
    want = RO.total_norm([e["g"] for e in entries])
    grads = Ptrs(In(f"g{i}", e["g"]) for i, e in enumerate(entries))
    out = held(eng, "pp_grad_norm", [grads, clens, count, 0.5 * want, Out("out", (2,)), None], "pp_grad_norm")["out"]
    norm, coef = float(out[0]), float(out[1])
    print(f"norm {norm:.9g}, float64 {want:.17g}, relative error {abs(norm - want) / want:.2e}; coef {coef:.9g}")
    assert abs(norm - want) <= 2.0 ** -23 * want and abs(coef - RO.clip_coef(want, 0.5 * want)) <= 4 * 2.0 ** -24
    half = np.array([0.5], np.float32)
    got = held(eng, "pp_scale_grads", [Ptrs(IO(f"g{i}", e["g"]) for i, e in enumerate(entries)), clens, count, In("coef", half), None], "pp_scale_grads")
    for i, e in enumerate(entries):
        assert np.array_equal((e["g"] * np.float32(0.5)).view(np.int32), got[f"g{i}"].cpu().numpy().view(np.int32)), i
    t, wd = 7, 1e-2
    one = np.array([1.0], np.float32)
    lists = [Ptrs(IO(f"p{i}", e["p"]) for i, e in enumerate(entries)), Ptrs(In(f"g{i}", e["g"]) for i, e in enumerate(entries)),
             Ptrs(IO(f"m{i}", e["m"]) for i, e in enumerate(entries)), Ptrs(IO(f"v{i}", e["v"]) for i, e in enumerate(entries))]
    got = held(eng, "pp_adam_step", lists + [clens, count, t, LR, 0.9, 0.999, 1e-8, wd, 0, In("coef", one), None], "pp_adam_step")
    x64, bar, _ = bars(entries, t, "Adam", wd)
    worst = np.zeros(3)
    for i, e in enumerate(entries):
        q = (got[f"p{i}"].cpu().numpy().astype(np.float64) - e["p"].astype(np.float64), got[f"m{i}"].cpu().numpy(), got[f"v{i}"].cpu().numpy())
        for k in range(3):
            worst[k] = max(worst[k], np.abs(q[k] - x64[i][k]).max())
    print(f"dp, exp_avg, exp_avg_sq: largest fraction of the bar {worst / bar}")
    assert (worst <= bar).all(), worst / bar
