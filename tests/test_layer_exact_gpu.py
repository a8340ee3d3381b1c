"""GPU (-m gpu): every convolution, upsampler and head kernel of the launch plan as a SINGLE layer (Engine.debug_layer ->
pp_debug_layer) against the plain numpy reference of tests/layer_ref.py.

(a) Exact cases.  Activations, weights, residual, bias and the prologue's scale / shift are small dyadic numbers (layer_ref's
    exactness condition: every partial sum of the contraction is exactly representable in fp32, whatever the order, the tile shape,
    the wave split or the MFMA shape), so the layer output must equal the reference BIT FOR BIT in every precision mode -- an
    indexing, masking, stride, packing or epilogue error is a mismatch, not "a bit more noise".  The per-channel sum of the epilogue's
    statistics is exact too; the sum of squares is an fp32 sum of n <= 1024 non-negative terms per partial: n 2^-24 relative.
    Grids (eight_20cm cells): 64 x 96 -> maps 32x48 / 16x24 / 8x12, every tile of every shape overhangs the map; 16 x 160 -> maps
    8x80 / 4x40 / 2x20, the 80 / 40 / 20 pixel tile widths divide the map and the maps are a few rows high.  Three frames with
    different data (and different scale / shift in the per-frame prologue): every frame stride is exercised.
    Winograd F(4x4,3x3) (`wino6`) divides by 6 and 24 and cannot be exact: where the fp32 plan picks it, the layer is held to
    layer_ref.winograd4_bound (componentwise, from the data) instead.
(b) Real-valued cases (standard normal inputs, raw prologue, the seeded network weights): the kernels round the operands
    deterministically (RNE) and accumulate K exact products in fp32; the reference rounds the same way and accumulates in float64.
    Per output element |gpu - ref| <= 2 K 2^-24 sum |x^||w^| (+ 3 2^-18 sum |x||w| for bf16x3: the dropped lo*lo term and the
    rounding of the two lo parts; + one fp16 ulp where the output tensor is fp16).  No share of elements may lie outside.
(c) The hook itself: bad arguments raise before anything is launched, inference is untouched by it."""
import ctypes

import numpy as np
import pytest
import torch

import layer_ref as R
import menu_cases as M
from conftest import load_pkg
from test_gpu_parity import C16_SHAPES  # the 13 tile shapes of conv16.hip, one list for both files

pytestmark = pytest.mark.gpu

# fp32 families that are exact on dyadic data: direct 3x3 stride 1 and 2 (masked-edge and exact shapes), the persistent 1x1 GEMM of
# the upsamplers and the head, Winograd F(2x2,3x3) -- wino_mfma and its one-wave-per-SIMD form wino4_mfma -- whose transforms only
# halve (two more bits of weight granularity, layer_ref.WINO_UNIT)
FP32_FORCED = ["k3s1 tw16 w1x4 t4x4", "k3s1 tw4 w2x2 t2x2", "k3s1 tw8 w2x2 t4x5", "k3s2 tw16 w1x4 t4x5", "k3s2 tw4 w2x2 t2x2", "k3s2 tw8 w2x2 t4x5",
               "g1x1", "wino tw8 w1x4 bx1 kc8", "wino tw4", "wino tw8 w2x4", "wino tw2", "wino4 tw4 bx2", "wino4 tw8 bx1"]
ALL_COMBOS = [(pre, res) for pre in R.PROLOGUES for res in (False, True)]
FORCED_COMBOS = [("frame", True), ("shared", False), ("raw", True)]
SUMSQ_REL = R.STAT_N * 2.0 ** -24


def small_cfg(synth, grid):
    gx, gy = R.ALL_GRIDS[grid]
    cfg = synth.load_config("eight_20cm")
    cfg["detection_range"] = [0.0, 0.0, -2.5, 0.2 * gx, 0.2 * gy, 8.5]
    cfg["max_voxels"] = 2000
    cfg["device"] = torch.device("cuda:0")
    return cfg


def make_engine(synth, grid, mode, sd):
    eng = load_pkg("engine").Engine(small_cfg(synth, grid), max_batch=R.NB, precision=mode)
    eng.load_state_dict(sd)
    assert (eng.H, eng.W) == (R.ALL_GRIDS[grid][0] // 2, R.ALL_GRIDS[grid][1] // 2) and eng.effective_precision() == mode
    return eng


@pytest.fixture(scope="module")
def exact_sd(synth):
    return R.exact_state_dict(synth.seeded_state_dict(0))


@pytest.fixture(scope="module")
def tally():
    """(mode -> (layer, tiling) pairs checked bit-exactly, mode -> largest |gpu - ref| / bound of the real-valued cases), printed at the end"""
    t = dict(exact={}, ratio={})
    yield t
    for mode in R.MODES:
        if mode in t["exact"] or mode in t["ratio"]:
            print(f"[layer exact] {mode}: {len(t['exact'].get(mode, ()))} (layer, tiling) pairs bit-exact"
                  + (f", largest |gpu - ref| / bound of the real-valued cases {t['ratio'][mode]:.3f}" if mode in t["ratio"] else ""))


def dev(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.array(a)).to(dtype).cuda()  # a copy: the shared cases are read-only


def host(t):
    return t.float().cpu().numpy()


def check_exact(eng, sd, index, grid, pre, with_res, tally=None, mode=None):
    """One exact case through the committed tiling of layer `index`; returns the tiling name."""
    t = eng.layer_tilings()[index]
    c = R.exact_case(sd, index, grid, pre, with_res)
    assert (t["kind"], t["cin"], t["cout"], t["stride"], t["up"], t["level"]) == tuple(c[k] for k in ("kind", "cin", "cout", "stride", "up", "level"))
    in_dt, out_dt = eng.layer_io_dtypes(index)
    what = (grid, index, t["tiling"], pre, with_res)
    args = dict(x=dev(c["x"], in_dt), res=dev(c["res"], out_dt), scale=dev(c["scale"]), shift=dev(c["shift"]))
    if pre == "raw" and t["wino"] in (4, 6):
        # wino4_mfma / wino6_mfma always normalise (a stride-1 convolution of the network always follows a norm): the hook refuses
        with pytest.raises(RuntimeError, match="raw prologue"):
            eng.debug_layer(index, **args)
        return t["tiling"]
    if t["kind"] == 2:
        got, st = eng.debug_layer(index, **args), None
    else:
        got, st = eng.debug_layer(index, stats=True, **args)
    torch.cuda.synchronize()
    if compare_exact(t, c, sd, index, out_dt, got, st, what) and tally is not None:
        tally["exact"].setdefault(mode, set()).add((grid, index, t["tiling"]))
    return t["tiling"]


_BOUNDS = {}


def compare_exact(t, c, sd, index, out_dt, got, st, what):
    """The comparison half of check_exact (test_layer_arena_gpu.py calls it on what it launched itself): the output(s) `got` and the
    statistics `st` of tiling entry `t` on exact case `c` against the case's reference.  True: bit for bit; False: a Winograd
    F(4x4,3x3) layer, held to its componentwise bound."""
    if t["kind"] == 2:
        for g, ref, name in zip(got, c["ref"], ("cls", "box", "dir")):
            assert np.array_equal(host(g), ref.astype(np.float32)), what + (name,)
        return True
    assert got.dtype == out_dt
    want = R.round_fp16(c["ref"]).astype(np.float32) if out_dt == torch.float16 else c["ref"].astype(np.float32)
    st = st.cpu().numpy()
    if t["wino"] == 6:  # Winograd F(4x4,3x3): not exact on any data (module docstring)
        if id(c) not in _BOUNDS:  # computed once per (shared, read-only) case; the entry keeps the case alive, so its id stays its own
            _BOUNDS[id(c)] = (c, R.winograd4_bound(R.prologue(c["x"], c["scale"], c["shift"]), R.layer_weights(sd, index)))
        bound = _BOUNDS[id(c)][1]
        err =np.abs(host(got).astype(np.float64) - c["ref"])
        assert (err <= bound).all(), what + (float((err / np.maximum(bound, 1e-300)).max()),)
        assert (np.abs(st[..., 0] - c["stats"][..., 0]) <= bound.sum(axis=(2, 3)) + SUMSQ_REL * np.abs(c["ref"]).sum(axis=(2, 3))).all(), what
        return False
    assert np.array_equal(host(got), want), what + (int((host(got) != want).sum()), float(np.abs(host(got) - want).max()))
    assert np.array_equal(st[..., 0], c["stats"][..., 0]), what + ("sum",)
    assert (np.abs(st[..., 1] - c["stats"][..., 1]) <= SUMSQ_REL * c["stats"][..., 1]).all(), what + ("sum of squares",)
    return True


# ------------------------------------------------------------------ (a) exact cases
@pytest.mark.parametrize("mode", R.MODES)
def test_exact_default_plan(mode, synth, exact_sd, tally):
    """Every layer of the plan at the tuner's own choice, every prologue, residual present and absent."""
    eng = make_engine(synth, "64x96", mode, exact_sd)
    til = eng.layer_tilings()
    assert len(til) == 20
    if mode != "fp32":  # every layer runs a kernel of the mode: conv16 (family 5) and the PREC instantiations of gemm1x1 (p<n> tag)
        assert all(t["wino"] == 5 if t["kind"] == 0 else f" p{eng.PRECISIONS[mode] if mode != 'fp16s' else 3}" in t["tiling"] for t in til), til
    if mode == "fp16s":
        assert [eng.layer_io_dtypes(i) for i in (0, 1, 4, 19)] == [(torch.float32, torch.float16), (torch.float16, torch.float16),
                                                                   (torch.float16, torch.float16), (torch.float16, torch.float32)]
    for index, t in enumerate(til):
        for pre, with_res in ALL_COMBOS:
            if with_res and t["kind"] != 0:
                continue
            check_exact(eng, exact_sd, index, "64x96", pre, with_res, tally, mode)
    w6 = sum(t["wino"] == 6 for t in til)
    print(f"[layer exact] default plan {mode}: {20 - w6} layers bit-exact in {len(ALL_COMBOS)} prologue / residual cases each"
          + (f", {w6} Winograd F(4x4) layers inside their componentwise bound" if w6 else ""))


@pytest.mark.parametrize("mode", ["bf16x3", "bf16", "fp16", "fp16s"])
@pytest.mark.parametrize("shape", C16_SHAPES)
def test_exact_conv16_forced_shape(shape, mode, synth, exact_sd, tally, monkeypatch):
    """Every tile shape of conv16.hip pinned, in every operand type, on every conv layer that takes it, on both grids.  fp16s: the fp16
    operand kernels on fp16 tensors (`h3`; the first conv reads fp32 and writes fp16, `h2`)."""
    monkeypatch.setenv("PP_FORCE_VARIANT", shape)
    ran = []
    for grid in sorted(R.GRIDS):
        eng = make_engine(synth, grid, mode, exact_sd)
        for index, t in enumerate(eng.layer_tilings()):
            if t["kind"] == 0 and shape in t["tiling"]:  # the shape really runs this layer (rows a multiple of its 64 / 128, its stride in the menu)
                tag = f"p3 h{2 if index == 0 else 3} " if mode == "fp16s" else f"p{eng.PRECISIONS[mode]} "
                assert t["wino"] == 5 and tag in t["tiling"]
                for pre, with_res in FORCED_COMBOS:
                    check_exact(eng, exact_sd, index, grid, pre, with_res, tally, mode)
                ran.append((grid, index))
        del eng
    assert ran, f"{shape} fits no conv layer on either grid"
    assert {g for g, _ in ran} == set(R.GRIDS)
    # ... and those are exactly the layers on which the library calls a conv16 entry of this shape legal (menu_cases.legal_table): with
    # test_menu_cpu's proof that the 13 shapes partition conv16's menus, every entry of every mode's menu has run wherever it can
    legal = {gk for key, rows in M.legal_table(mode).items() if key.startswith("k3") for n, where in rows if shape in n for gk in where if gk[0] in R.GRIDS}
    assert set(ran) == legal, (sorted(set(ran) ^ legal))
    print(f"[layer exact] conv16 {shape} {mode}: {len(ran)} layers bit-exact")


@pytest.mark.parametrize("force", FP32_FORCED)
def test_exact_fp32_forced_family(force, synth, exact_sd, tally, monkeypatch):
    monkeypatch.setenv("PP_FORCE_VARIANT", force)
    ran = []
    for grid in sorted(R.GRIDS):
        eng = make_engine(synth, grid, "fp32", exact_sd)
        for index, t in enumerate(eng.layer_tilings()):
            if force in t["tiling"]:
                for pre, with_res in FORCED_COMBOS:
                    if with_res and t["kind"] != 0:
                        continue
                    check_exact(eng, exact_sd, index, grid, pre, with_res, tally, "fp32")
                ran.append((grid, index))
        del eng
    assert ran, f"{force} fits no layer on either grid"
    print(f"[layer exact] fp32 {force}: {len(ran)} layers bit-exact")


@pytest.mark.parametrize("mode", ["fp32", "fp16", "fp16s"])
def test_exact_sparse_twin_of_the_first_conv(mode, synth, exact_sd, tally):
    """Layer 0 given the pillar map + PFN rows (the tiling's sparse twin) and the same frames as a dense scattered canvas: both equal the
    reference, hence each other, bit for bit.  Frame 1 holds no pillar."""
    grid = "64x96"
    gx, gy = R.GRIDS[grid]
    eng = make_engine(synth, grid, mode, exact_sd)
    rng = np.random.default_rng(21)
    P = eng.max_voxels
    feat = (rng.integers(-7, 8, (R.NB, P, 64)) * 0.25).astype(np.float32)
    pmap = np.full((R.NB, gx, gy), -1, np.int32)
    canvas = np.zeros((R.NB, 64, gx, gy), np.float32)
    for f, n in ((0, 700), (2, 1500)):  # frame 1 stays empty; rows beyond a frame's count are never referenced
        cells = rng.choice(gx * gy, n, replace=False)
        ids = rng.permutation(P)[:n]
        pmap[f].reshape(-1)[cells] = ids
        canvas[f].reshape(64, -1)[:, cells] = feat[f, ids].T
    pmap[0, 0, :] = -1  # an empty border row and column
    canvas[0, :, 0, :] = 0
    pmap[0, :, gy - 1] = -1
    canvas[0, :, :, gy - 1] = 0
    ref = R.layer(0, canvas, R.layer_weights(exact_sd, 0), "fp32", stride=2)
    assert R.exactness_margin(R.layer(0, canvas, R.layer_weights(exact_sd, 0), "fp32", stride=2, magnitude=True)) < 1.0
    assert not ref[1].any() and ref[0].any() and ref[2].any()
    in_dt, out_dt = eng.layer_io_dtypes(0)
    assert in_dt == torch.float32
    want = R.round_fp16(ref).astype(np.float32) if out_dt == torch.float16 else ref.astype(np.float32)
    sparse, st_s = eng.debug_layer(0, pmap=dev(pmap, torch.int32), feat=dev(feat), stats=True)
    dense, st_d = eng.debug_layer(0, x=dev(canvas), stats=True)
    torch.cuda.synchronize()
    assert np.array_equal(host(dense), want), "dense canvas"
    assert np.array_equal(host(sparse), want), "pillar map + PFN rows"
    for st in (st_s, st_d):
        st = st.cpu().numpy()
        assert np.array_equal(st[..., 0], R.channel_stats(ref)[..., 0]) and not st[1].any()
        assert (np.abs(st[..., 1] - R.channel_stats(ref)[..., 1]) <= SUMSQ_REL * R.channel_stats(ref)[..., 1]).all()
    tally["exact"].setdefault(mode, set()).add((grid, 0, eng.layer_tilings()[0]["tiling"] + " sparse"))


# ------------------------------------------------------------------ (b) real-valued cases
REAL_LAYERS = (0, 1, 5, 6, 12, 13, 4, 11, 18, 19)  # a stride-2 and a stride-1 conv per level, the three upsamplers, the head


@pytest.mark.parametrize("mode", R.MODES[1:])
def test_real_valued_layers_within_the_derived_bound(mode, synth, tally):
    sd = synth.seeded_state_dict(0)
    eng = make_engine(synth, "64x96", mode, sd)
    til = eng.layer_tilings()
    worst = 0.0
    for index in REAL_LAYERS:
        t, L = til[index], R.plan_shapes(*R.GRIDS["64x96"])[index]
        in_dt, out_dt = eng.layer_io_dtypes(index)
        x = np.random.default_rng(100 + index).standard_normal((R.NB, L["cin"], L["hin"], L["win"])).astype(np.float32)
        if in_dt == torch.float16:
            x = R.round_fp16(x)  # the tensor the kernel reads IS fp16
        w = R.layer_weights(sd, index)
        ref = R.layer(L["kind"], x, w, mode, stride=L["stride"])
        mag = R.layer(L["kind"], x, w, mode, stride=L["stride"], magnitude=True)
        K = L["cin"] * (9 if L["kind"] == 0 else 1)
        got = eng.debug_layer(index, x=dev(x, in_dt))
        torch.cuda.synchronize()
        for g, r, m in zip(got if L["kind"] == 2 else (got,), ref if L["kind"] == 2 else (ref,), mag if L["kind"] == 2 else (mag,)):
            bound = 2 * K * 2.0 ** -24 * m
            if mode == "bf16x3":
                bound = bound + 3 * 2.0 ** -18 * m
            if g.dtype == torch.float16:
                r = R.round_fp16(r)
                bound = bound + 2.0 ** -10 * np.abs(r)  # both sides round to nearest: at most one fp16 ulp apart on top
            ratio = np.abs(host(g).astype(np.float64) - r) / bound
            worst = max(worst, float(ratio.max()))
            assert (ratio <= 1.0).all(), (mode, index, t["tiling"], float(ratio.max()), int((ratio > 1).sum()))
    tally["ratio"][mode] = worst
    print(f"[layer real] {mode}: {len(REAL_LAYERS)} layers, largest |gpu - ref| / bound {worst:.3f}")


# ------------------------------------------------------------------ (c) the hook itself
def test_hook_rejects_bad_arguments_before_any_launch(synth, exact_sd):
    eng = make_engine(synth, "64x96", "fp32", exact_sd)
    c = R.exact_case(exact_sd, 1, "64x96", "shared", True)
    x, res, sc, sh = dev(c["x"]), dev(c["res"]), dev(c["scale"]), dev(c["shift"])
    good = eng.debug_layer(1, x=x, res=res, scale=sc, shift=sh)
    torch.cuda.synchronize()
    for bad in (lambda: eng.debug_layer(20, x=x), lambda: eng.debug_layer(-1, x=x), lambda: eng.debug_layer(1, x=x[:, :, :-1]),
                lambda: eng.debug_layer(1, x=torch.cat([x, x])), lambda: eng.debug_layer(1, x=x.half()), lambda: eng.debug_layer(1, x=x.cpu()),
                lambda: eng.debug_layer(1, x=x, scale=sc), lambda: eng.debug_layer(4, x=x, res=res), lambda: eng.debug_layer(1),
                lambda: eng.debug_layer(1, pmap=torch.zeros((3, 64, 96), dtype=torch.int32).cuda(), feat=torch.zeros((3, 2000, 64)).cuda()),
                lambda: eng.debug_layer(19, x=torch.zeros((3, 320, 32, 48)).cuda(), stats=True)):
        with pytest.raises((ValueError, TypeError)):
            bad()
    # the C entry validates on its own, whatever the binding did: every call returns an error code and launches nothing
    lib, p = eng.lib, lambda t: ctypes.c_void_p(t.data_ptr())
    out = torch.full_like(good, 7.0)
    calls = [(99, 3, p(x), None, 0, None, None, None, None, p(out), None, None, None), (1, 0, p(x), None, 0, None, None, None, None, p(out), None, None, None),
             (1, 4, p(x), None, 0, None, None, None, None, p(out), None, None, None), (1, 3, None, None, 0, None, None, None, None, p(out), None, None, None),
             (1, 3, p(x), None, 0, None, None, None, None, None, None, None, None), (1, 3, p(x), None, 1, p(sc), None, None, None, p(out), None, None, None),
             (1, 3, p(x), None, 0, p(sc), p(sh), None, None, p(out), None, None, None), (1, 3, p(x), None, 3, p(sc), p(sh), None, None, p(out), None, None, None),
             (4, 3, p(x), p(res), 0, None, None, None, None, p(out), None, None, None), (1, 3, None, None, 0, None, None, p(x), p(x), p(out), None, None, None),
             (0, 3, p(x), None, 0, None, None, p(x), p(x), p(out), None, None, None), (19, 3, p(x), None, 0, None, None, None, None, p(out), None, None, None),
             (1, 3, p(x), None, 0, None, None, None, None, p(out), p(out), p(out), None), (19, 3, p(x), None, 0, None, None, None, None, p(out), p(out), p(out), p(out))]
    for a in calls:
        assert lib.pp_debug_layer(eng.ctx, *a, None) != 0, a
        assert lib.pp_last_error(eng.ctx)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    again = eng.debug_layer(1, x=x, res=res, scale=sc, shift=sh)  # the next valid call works
    torch.cuda.synchronize()
    assert torch.equal(again, good) and np.array_equal(host(good), c["ref"].astype(np.float32))


@pytest.mark.parametrize("mode", ["fp32", "fp16s"])
def test_hook_leaves_inference_unchanged(mode, synth, exact_sd):
    """A frame inferred before and after debug_layer calls (statistics, the head, the sparse form) is identical: logits and detections."""
    sd = synth.seeded_state_dict(0, cls_bias=-3.0)
    eng = make_engine(synth, "64x96", mode, sd)
    rng = np.random.default_rng(4)
    pts = torch.from_numpy(np.concatenate([rng.uniform(0.0, 12.8, (4000, 1)), rng.uniform(0.0, 19.2, (4000, 1)), rng.uniform(-2.0, 2.0, (4000, 1)),
                                           rng.uniform(0.0, 1.0, (4000, 1))], axis=1).astype(np.float32)).cuda()

    def frame():
        det, cnt = eng.infer_frame(pts)
        out = [det.clone(), cnt.clone()] + [eng.fetch(0, k).clone() for k in ("cls", "box", "dir", "rpn")]
        torch.cuda.synchronize()
        return out

    before = frame()
    assert int(before[1][0]) >= 0 and bool(torch.isfinite(before[2]).all())
    det, cnt = eng.infer_frame(pts)  # the hook runs between a pass and the reads of its (possibly deferred) head outputs
    for index in (0, 1, 4, 18, 19):
        L = R.plan_shapes(*R.GRIDS["64x96"])[index]
        in_dt, out_dt = eng.layer_io_dtypes(index)
        x = torch.randn((R.NB, L["cin"], L["hin"], L["win"]), device="cuda").to(in_dt)
        aff = dict(scale=torch.rand((R.NB, L["cin"]), device="cuda"), shift=torch.randn((R.NB, L["cin"]), device="cuda"))
        eng.debug_layer(index, x=x, stats=L["kind"] != 2, **aff)
    eng.debug_layer(0, pmap=torch.full((R.NB, 64, 96), -1, dtype=torch.int32, device="cuda"), feat=torch.zeros((R.NB, eng.max_voxels, 64), device="cuda"))
    mid = [det, cnt] + [eng.fetch(0, k) for k in ("cls", "box", "dir", "rpn")]
    torch.cuda.synchronize()
    after = frame()
    for a, b, c in zip(before, mid, after):
        assert torch.equal(a, b) and torch.equal(a, c)
