"""GPU (-m gpu): a layer's result depends on its tensors and on nothing else.

The single-layer tests reach the kernels through Engine.debug_layer / debug_head_cls, which stage the input in a zeroed buffer and take
the outputs from torch.empty.  The kernels read `in` through unbounded buffer descriptors, fetch for masked-out lanes too and prefetch
ahead of the compute side -- and zeros are exactly what 3x3 zero padding should give, so a broken top / bottom / row-end mask on the
first plane of the first frame or the last plane of the last frame reads the staging buffer and is bit-exact by coincidence.  Here the
C entries are called directly (eng.lib) on tensors that sit in arenas (tests/arena.py): `in` with exactly the slack include/pp_hip.h
grants it (IN_FRONT / IN_BEHIND bytes), every other argument with none, all surrounded by bands the test owns.  Each case runs once
per fill of the surroundings -- zeros, quiet NaNs, and finite +-2^40 (fp16 +-2^14) of alternating sign: the prologue's ReLU is a max /
med3 that drops a NaN operand, so a leaked NaN can come out as 0, the padding value; a leaked +-2^40 survives relu(x * scale + shift)
for one of the two signs and wrecks the sum -- and must give
  (a) the reference: compare_exact of test_layer_exact_gpu.py (bit for bit; Winograd F(4x4,3x3) inside its bound),
  (b) the same bits under every fill, output and statistics, wino6 included,
  (c) no byte changed outside the tensors, inputs included (outputs and their surroundings start as the byte 0xA5),
  (d) no output element left at 0xA5: checked where the reference provably differs from that pattern -- the bit-exact cases, after a
      CPU-side check of the reference.  A wino6 output left at the pattern fails (a) wherever (d) could be decided at all.  The
      statistics are sums of fp32 values held in fp64: 0 or at least 2^-149 in magnitude, never the pattern's 2^-421.
The zero-fill run of a case is held to (a) and (d), the other two to (b) -- identical bits compare identically -- and all three to (c).
Cases: every entry of every fp32 menu, the 13 conv16 shapes and both gemm1x1 tilings in every 16-bit mode, the strip tilings, the
cls-only head pass, the sparse first conv and the tile-skipping launches.  One engine per (grid, pinned tilings) serves all fills."""
import ctypes
import time

import numpy as np
import pytest
import torch

import arena as A
import layer_ref as R
import menu_cases as M
import tile_skip_ref as T
from test_gpu_parity import C16_SHAPES
from test_layer_exact_gpu import compare_exact, dev, exact_sd, host, make_engine  # noqa: F401 (fixture)
from test_menu_exact_gpu import G1X1_KEYS
from test_tile_skip_gpu import H as TS_H, W as TS_W, NTX, NTY, forced_engine, make_cfg

pytestmark = pytest.mark.gpu

# include/pp_hip.h, pp_debug_layer: `in` is readable this many bytes in front of its first and behind its last element
IN_FRONT, IN_BEHIND = 256, 256


def ptr(a):
    return None if a is None else ctypes.c_void_p(a.ptr)


def combos(t):
    """prologue / residual cases of a layer: raw without residual (zero staging hides a mask error exactly) and the per-frame prologue,
    with the residual where the layer takes one"""
    return [("raw", False), ("frame", t["kind"] == 0)]


class Run:
    """One launch of a C entry on arena tensors.  ins / outs: {argument name: Arena}."""

    def __init__(self, eng, fill, shapes, x=None, res=None, scale=None, shift=None, pmap=None, feat=None, active=None):
        self.eng, self.fill = eng, fill
        given = dict(res=res, scale=scale, shift=shift, pmap=pmap, feat=feat, active=active)
        self.ins = {k: A.place(v, 0, 0, fill) for k, v in given.items() if v is not None}  # the header grants these no slack
        if x is not None:
            self.ins["in"] = A.place(x, IN_FRONT, IN_BEHIND, fill)
        self.outs = {k: A.place_out(shape, dt) for k, (shape, dt) in shapes.items()}
        self.pre_mode = 0 if scale is None else (2 if scale.dim() == 2 else 1)

    def arg(self, name):
        return ptr(self.ins.get(name) or self.outs.get(name))

    def layer(self, index, skip_k=0):
        a = self.arg
        head = (self.eng.ctx, index, R.NB, a("in"), a("res"), self.pre_mode, a("scale"), a("shift"), a("pmap"), a("feat"),
                a("out"), a("out_box"), a("out_dir"), a("stats"))
        if skip_k:
            rc = self.eng.lib.pp_debug_layer_skip(*head, a("active"), skip_k, None)
        else:
            rc = self.eng.lib.pp_debug_layer(*head, None)
        torch.cuda.synchronize()
        return rc

    def head_cls(self):
        a = self.arg
        rc = self.eng.lib.pp_debug_head_cls(self.eng.ctx, R.NB, a("in"), self.pre_mode, a("scale"), a("shift"), a("out"), None)
        torch.cuda.synchronize()
        return rc

    def bits(self):
        """{output name: its elements as integers} -- what (b) compares"""
        return {k: o.words().clone() for k, o in self.outs.items()}

    def check_untouched(self, what):
        for k, a in {**self.ins, **self.outs}.items():
            assert A.untouched(a), what + (self.fill, f"bytes outside `{k}` changed")  # (c)


def out_shapes(eng, t, out_dt, stats=True):
    """{output argument: (shape, type)} of tiling entry t (eng.layer_tilings()[index]; out_dt = eng.layer_io_dtypes(index)[1])"""
    h, w = (eng.H >> t["level"]) * t["up"], (eng.W >> t["level"]) * t["up"]
    if t["kind"] == 2:
        return dict(out=((R.NB, eng.A, 1), torch.float32), out_box=((R.NB, eng.A, 7), torch.float32), out_dir=((R.NB, eng.A, 2), torch.float32))
    s = dict(out=((R.NB, t["cout"], h, w), out_dt))
    if stats:
        s["stats"] = ((R.NB, t["cout"], 2), torch.float64)
    return s


def check_fills(make_run, launch, t, c, sd, index, out_dt, what):
    """(a) - (d) of one case: make_run(fill) -> Run, launch(run) -> rc.  The zero-fill run comes first and is held to (a) and (d); the
    NaN and the finite run must reproduce its outputs and statistics bit for bit (b), which is (a) and (d) for them as well -- the
    same bits compare the same -- and every run to (c)."""
    assert A.FILLS[0] == "zeros"
    base = None
    for fill in A.FILLS:
        run = make_run(fill)
        rc = launch(run)
        assert rc == 0, what + (fill, run.eng.lib.pp_last_error(run.eng.ctx))
        if base is None:
            got = tuple(run.outs[k].t for k in ("out", "out_box", "out_dir") if k in run.outs) if t["kind"] == 2 else run.outs["out"].t
            st = run.outs["stats"].t if "stats" in run.outs else None
            exact = compare_exact(t, c, sd, index, out_dt, got, st, what + (fill,))  # (a)
            if exact:  # (d): the reference holds the pattern nowhere, so neither may the output
                refs = c["ref"] if t["kind"] == 2 else (c["ref"],)
                for k, ref in zip(("out", "out_box", "out_dir"), refs):
                    o = run.outs[k]
                    assert reference_is_pattern_free(ref, o.t.dtype)
                    assert o.stale() == 0, what + (fill, f"{o.stale()} elements of `{k}` never stored")
            if st is not None:
                assert run.outs["stats"].stale() == 0, what + (fill, "statistics never stored")
            base = run.bits()
        else:
            for k, b in ((k, o.words()) for k, o in run.outs.items()):
                assert torch.equal(b, base[k]), what + (fill, f"`{k}` differs from the zero-fill run", int((b != base[k]).sum()))  # (b)
        run.check_untouched(what)  # (c)


_PATTERN_FREE = {}


def reference_is_pattern_free(ref, dtype):
    """CPU side of (d), once per reference array and output type: no element of the reference, as stored, is the 0xA5 pattern"""
    key = (id(ref), dtype)
    if key not in _PATTERN_FREE:
        want = R.round_fp16(ref).astype(np.float16) if dtype == torch.float16 else ref.astype(np.float32)
        _PATTERN_FREE[key] = (ref, A.pattern_free(want, want.dtype.itemsize))
    return _PATTERN_FREE[key][1]


def arena_case(eng, sd, index, grid, pre, with_res):
    """One exact case of layer `index` under every fill; returns the tiling name."""
    t = eng.layer_tilings()[index]
    c = R.exact_case(sd, index, grid, pre, with_res)
    assert (t["kind"], t["cin"], t["cout"], t["stride"], t["up"], t["level"]) == tuple(c[k] for k in ("kind", "cin", "cout", "stride", "up", "level"))
    in_dt, out_dt = eng.layer_io_dtypes(index)
    what = (grid, index, t["tiling"], pre, with_res)
    args = dict(x=dev(c["x"], in_dt), res=dev(c["res"], out_dt), scale=dev(c["scale"]), shift=dev(c["shift"]))
    shapes = out_shapes(eng, t, out_dt)
    if pre == "raw" and t["wino"] in (4, 6):  # wino4_mfma / wino6_mfma always normalise: the entry refuses and launches nothing
        run = Run(eng, "poison", shapes, **args)
        assert run.layer(index) != 0 and b"raw prologue" in eng.lib.pp_last_error(eng.ctx)
        run.check_untouched(what)
        assert all(o.stale() == o.t.numel() for o in run.outs.values())
        return t["tiling"]
    check_fills(lambda fill: Run(eng, fill, shapes, **args), lambda run: run.layer(index), t, c, sd, index, out_dt, what)
    return t["tiling"]


def run_slot(mode, i, keys, synth, sd, monkeypatch):
    """test_menu_exact_gpu.run_slot with arena_case in place of check_exact: entry i of the menus `keys` pinned, one engine per grid,
    the pinned tilings run exactly the layers the CPU table calls legal.  Returns {name: layers run}."""
    names = M.slot_names(mode, i, keys)
    if not names:
        return {}
    monkeypatch.setenv("PP_FORCE_VARIANT", ";".join(names.values()))
    expect = M.slot_layers(mode, i, R.GRIDS, keys)
    ran = {name: 0 for name in names.values()}
    t0 = time.time()
    for grid in sorted(R.GRIDS):
        eng = make_engine(synth, grid, mode, sd)
        for index, t in enumerate(eng.layer_tilings()):
            want = expect.get((grid, index))
            if want is None:
                continue
            assert t["tiling"] == want, (grid, index, t["tiling"], want)
            for pre, with_res in combos(t):
                assert arena_case(eng, sd, index, grid, pre, with_res) == want
            ran[want] += 1
        del eng
    never = {n for (m, key, n) in M.NEVER_LEGAL if m == mode}
    for name, n in ran.items():
        assert n > 0 or name in never, f"{name} ran on no layer"
    print(f"[arena slot] {mode} slot {i}: " + ", ".join(f"{name} x{n}" for name, n in ran.items()) + f" ({time.time() - t0:.1f} s)")
    return ran


# ------------------------------------------------------------------ the helper itself
def test_arena_layout_and_fills():
    x = torch.arange(3 * 5 * 7, dtype=torch.float32, device="cuda").reshape(3, 5, 7)
    for fill, word, half in (("zeros", (0, 0), (0, 0)), ("nan", (0x7FC00BAD,) * 2, (0x7E01,) * 2), ("poison", (0x53800000, 0xD3800000), (0x7400, 0xF400))):
        a = A.place(x, 256, 512, fill)
        assert a.t.data_ptr() % 512 == 256 and torch.equal(a.t, x) and a.lo >= A.BAND + 256 and a.buf.numel() - a.hi >= A.BAND + 512
        w = a.buf.view(torch.int32).cpu().numpy().view(np.uint32)
        outside = np.r_[w[:a.lo // 4], w[a.hi // 4 + 1:]]  # (105 floats: the word behind the tensor is odd, start the tail at an even one)
        assert (outside[0::2] == word[0]).all() and (outside[1::2] == word[1]).all()
        b = A.place(x.half(), 0, 0, fill)
        hw = b.buf.view(torch.int16).cpu().numpy().view(np.uint16)
        assert (hw[:b.lo // 2:2] == half[0]).all() and (hw[1:b.lo // 2:2] == half[1]).all() and torch.equal(b.t, x.half())
        assert A.untouched(a) and A.untouched(b)
        if fill == "poison":
            v = a.buf[:a.lo].view(torch.float32)
            assert float(v[0]) == 2.0 ** 40 and float(v[1]) == -2.0 ** 40 and float(b.buf[:b.lo].view(torch.float16)[1]) == -2.0 ** 14
        if fill == "nan":
            assert bool(torch.isnan(a.buf[:a.lo].view(torch.float32)).all()) and bool(torch.isnan(b.buf[:b.lo].view(torch.float16)).all())
        a.buf[a.hi] += 1  # one byte behind the tensor
        b.buf[b.lo - 1] += 1  # one byte in front
        assert not A.untouched(a) and not A.untouched(b)
    big = A.place(torch.zeros((3, 64, 32, 48), device="cuda"), 0, 0, "zeros")
    assert big.lo >= 64 * 32 * 48 * 4  # a band holds a frame
    o = A.place_out((3, 4, 2), torch.float64)
    assert o.stale() == 24 and A.untouched(o)
    o.t[1:] = 0.0
    assert o.stale() == 8 and A.untouched(o)
    assert A.pattern_free(np.zeros(4, np.float32), 4) and not A.pattern_free(np.array([0xA5A5A5A5], np.uint32).view(np.float32), 4)


# ------------------------------------------------------------------ every menu entry
@pytest.mark.parametrize("i", range(M.MENU_SLOTS))
def test_arena_menu_slot(i, synth, exact_sd, monkeypatch):
    """Entry i of every fp32 menu: direct 3x3, Winograd F(2x2) and F(4x4), the 1x1 GEMM of the upsamplers and the head."""
    ran = run_slot("fp32", i, None, synth, exact_sd, monkeypatch)
    assert bool(ran) == (i < max(len(rows) for rows in M.legal_table("fp32").values()))


@pytest.mark.parametrize("mode", ["bf16x3", "bf16", "fp16", "fp16s"])
@pytest.mark.parametrize("shape", C16_SHAPES)
def test_arena_conv16_shape(shape, mode, synth, exact_sd, monkeypatch):
    """Every tile shape of conv16.hip in every operand type on every conv layer that takes it.  fp16s: fp16 tensors, the slack of `in`
    is counted in bytes, not elements."""
    monkeypatch.setenv("PP_FORCE_VARIANT", shape)
    ran = []
    for grid in sorted(R.GRIDS):
        eng = make_engine(synth, grid, mode, exact_sd)
        for index, t in enumerate(eng.layer_tilings()):
            if t["kind"] == 0 and shape in t["tiling"]:
                assert t["wino"] == 5
                for pre, with_res in combos(t):
                    arena_case(eng, exact_sd, index, grid, pre, with_res)
                ran.append((grid, index))
        del eng
    legal = {gk for key, rows in M.legal_table(mode).items() if key.startswith("k3") for n, where in rows if shape in n for gk in where if gk[0] in R.GRIDS}
    assert ran and set(ran) == legal, sorted(set(ran) ^ legal)


@pytest.mark.parametrize("i", (0, 1))
@pytest.mark.parametrize("mode", R.MODES[1:])
def test_arena_g1x1_16bit_slot(mode, i, synth, exact_sd, monkeypatch):
    """Both gemm1x1 tilings of the three upsamplers and the head in every 16-bit mode (fp16s: on fp16 tensors)."""
    ran = run_slot(mode, i, G1X1_KEYS, synth, exact_sd, monkeypatch)
    assert len(ran) == 4 and all(n.startswith("g1x1") for n in ran) and all(n >= 2 for n in ran.values()), ran


@pytest.mark.parametrize("strips", ["2", "0"])
@pytest.mark.parametrize("family", ["wino4 tw4 bx2", "wino6 tw4"])
def test_arena_strip_tilings(family, strips, synth, exact_sd, monkeypatch):
    """The four forms of test_exact_strip_tilings on the 36 x 44 map: main tiles + right and bottom strips, and the rounded-up masked form."""
    grid = next(iter(R.STRIP_GRID))
    monkeypatch.setenv("PP_FORCE_VARIANT", family)
    monkeypatch.setenv("PP_W4_STRIPS", strips)
    eng = make_engine(synth, grid, "fp32", exact_sd)
    til = eng.layer_tilings()
    layers = [k for k, t in enumerate(til) if t["kind"] == 0 and t["stride"] == 1 and t["level"] == 0 and family in t["tiling"]]
    assert layers == [1, 2, 3] and (eng.H, eng.W) == (36, 44), (layers, til[1:4])
    for k in layers:
        for pre, with_res in combos(til[k]):  # raw: refused by both families, nothing launched
            assert family in arena_case(eng, exact_sd, k, grid, pre, with_res)


# ------------------------------------------------------------------ the cls-only head pass
@pytest.mark.parametrize("pd", ["pd8", "pd10", "pd4"])
def test_arena_head_cls(pd, synth, exact_sd, monkeypatch):
    """pp_debug_head_cls at each ring depth on both gemm1x1 head images: `in` padded like pp_debug_layer's, cls_out alone written."""
    heads = [n for n, _ in M.legal_table("fp32")["head"] if n.startswith("g1x1")]
    assert len(heads) == 2
    head_t = dict(kind=2)
    for head_name in heads:
        monkeypatch.setenv("PP_FORCE_VARIANT", f"g1x1 cls {pd};{head_name}")
        for grid in sorted(R.GRIDS):
            eng = make_engine(synth, grid, "fp32", exact_sd)
            assert f" {pd} " in eng.head_cls_tiling() and eng.layer_tilings()[19]["tiling"] == head_name
            for pre in ("raw", "frame"):
                c = R.exact_case(exact_sd, 19, grid, pre, False)
                args = dict(x=dev(c["x"]), scale=dev(c["scale"]), shift=dev(c["shift"]))
                shapes = dict(out=((R.NB, eng.A, 1), torch.float32))
                cls_c = dict(ref=c["ref"][:1])  # compare_exact zips outputs with references: the cls part alone
                check_fills(lambda fill: Run(eng, fill, shapes, **args), lambda run: run.head_cls(), head_t, cls_c, exact_sd, 19,
                            torch.float32, (pd, head_name, grid, pre))
            del eng


# ------------------------------------------------------------------ the sparse first conv
@pytest.mark.parametrize("mode", ["fp32", "fp16", "fp16s"])
def test_arena_sparse_first_conv(mode, synth, exact_sd):
    """Layer 0 on the pillar map + PFN rows (test_exact_sparse_twin_of_the_first_conv's data; frame 1 holds no pillar).  Under the NaN
    and the finite fill the PFN rows no map cell references hold the fill as well: the result does not move."""
    grid = "64x96"
    gx, gy = R.GRIDS[grid]
    eng = make_engine(synth, grid, mode, exact_sd)
    rng = np.random.default_rng(21)
    P = eng.max_voxels
    feat = (rng.integers(-7, 8, (R.NB, P, 64)) * 0.25).astype(np.float32)
    pmap = np.full((R.NB, gx, gy), -1, np.int32)
    canvas = np.zeros((R.NB, 64, gx, gy), np.float32)
    used = np.zeros((R.NB, P), bool)
    for f, n in ((0, 700), (2, 1500)):
        cells = rng.choice(gx * gy, n, replace=False)
        ids = rng.permutation(P)[:n]
        pmap[f].reshape(-1)[cells] = ids
        canvas[f].reshape(64, -1)[:, cells] = feat[f, ids].T
    pmap[0, 0, :] = -1
    canvas[0, :, 0, :] = 0
    pmap[0, :, gy - 1] = -1
    canvas[0, :, :, gy - 1] = 0
    for f in range(R.NB):
        used[f, pmap[f][pmap[f] >= 0]] = True
    assert not used[1].any() and 0 < used[0].sum() < P and 0 < used[2].sum() < P
    w = R.layer_weights(exact_sd, 0)
    ref = R.layer(0, canvas, w, "fp32", stride=2)
    assert R.exactness_margin(R.layer(0, canvas, w, "fp32", stride=2, magnitude=True)) < 1.0 and not ref[1].any() and ref[0].any() and ref[2].any()
    c = dict(ref=ref, stats=R.channel_stats(ref), x=canvas, scale=None, shift=None)
    t = eng.layer_tilings()[0]
    in_dt, out_dt = eng.layer_io_dtypes(0)
    assert in_dt == torch.float32 and t["wino"] != 6
    pmap_d, unused = dev(pmap, torch.int32), torch.from_numpy(~used).cuda()

    def make_run(fill):
        feat_d = dev(feat)
        if fill != "zeros":
            feat_d.view(torch.uint8).view(R.NB, P, 256)[unused] = A.fill_words(fill, 4, 256, feat_d.device)
            assert torch.equal(feat_d[~unused], dev(feat)[~unused]) and (fill != "nan" or bool(torch.isnan(feat_d[1]).all()))
        return Run(eng, fill, out_shapes(eng, t, out_dt), pmap=pmap_d, feat=feat_d)

    check_fills(make_run, lambda run: run.layer(0), t, c, exact_sd, 0, out_dt, (grid, 0, t["tiling"] + " sparse", mode))


# ------------------------------------------------------------------ tile skipping
def test_arena_tile_skip(synth, monkeypatch):
    """pp_debug_layer_skip, skip_k = 1..3, on test_tile_skip_gpu.py's level-0 map and data (frames empty / one pixel / full, the inputs
    of layers 2 and 3 produced by the previous layers): the listed launch plus the fill kernel, which writes `out` as well, on arena
    tensors.  The reference is the dense launch of the same layer (bit for bit, as test_single_layers_bit_for_bit holds it)."""
    eng = forced_engine(synth, make_cfg(synth), R.NB)
    assert (eng.H, eng.W) == (TS_H, TS_W) and all(eng.layer_tilings()[i]["wino"] == 6 for i in (1, 2, 3))
    eng.set_tile_skip(True)
    rng = np.random.default_rng(11)
    act = np.zeros((R.NB, TS_H, TS_W), bool)
    act[1, 24, 40] = True
    act[2] = True
    const = rng.integers(0, 8, (R.NB, 64, 1, 1)).astype(np.float32) * 0.25
    x0 = dev(np.where(act[:, None], R.exact_activations(rng, (R.NB, 64, TS_H, TS_W)).astype(np.float32), const).astype(np.float32))
    bitmap = dev(act.astype(np.uint8), torch.uint8)
    aff = [tuple(dev(a) for a in R.exact_affine(rng, (R.NB, 64))) for _ in range(3)]
    ins = {1: (x0, None)}
    for k in (1, 2, 3):
        x, res = ins[k]
        sc, sh = aff[k - 1]
        dense, st_d = eng.debug_layer(k, x=x, res=res, scale=sc, shift=sh, stats=True)
        torch.cuda.synchronize()
        assert not eng.tile_skip_active() and A.pattern_free(host(dense), 4)
        nskip = [int(T.tile_flags(act[f])[k - 1].sum()) for f in range(R.NB)]
        assert nskip[0] == NTY * NTX and nskip[2] == 0
        base = None
        for fill in A.FILLS:
            run = Run(eng, fill, out_shapes(eng, eng.layer_tilings()[k], torch.float32), x=x, res=res, scale=sc, shift=sh, active=bitmap)
            what = (k, fill)
            assert run.layer(k, skip_k=k) == 0, what + (eng.lib.pp_last_error(eng.ctx),)
            assert eng.tile_skip_active()
            assert torch.equal(run.outs["out"].t, dense), what + ("listed launch + fill against the dense launch",)  # (a)
            rel = ((run.outs["stats"].t - st_d).abs() / torch.maximum(st_d.abs(), run.outs["stats"].t.abs()).clamp_min(1e-300)).max()
            assert float(rel) <= 1e-12, what + (float(rel),)
            bits = run.bits()
            base = base or bits
            assert all(torch.equal(bits[n], base[n]) for n in bits), what + ("differs from the zero-fill run",)  # (b)
            run.check_untouched(what)  # (c)
            assert run.outs["out"].stale() == 0 and run.outs["stats"].stale() == 0, what  # (d)
        ins[k + 1] = (dense, x0 if k == 1 else dense)
