"""GPU (-m gpu): EVERY tiling of every menu the tuner chooses from, pinned and run as a single layer against the exact-arithmetic
reference of tests/layer_ref.py -- not only the tilings the tuner happens to pick on the test maps, nor a hand-written list.

The menus come from the library (engine.menu_names -> pp_menu_names), the parametrisation is static: slot i pins entry i of every menu
that has one (PP_FORCE_VARIANT = their full names; the menus of the layer kinds share no name, test_menu_cpu.py).  menu_cases.legal_table
says on which (grid, layer) each entry is legal; the test asserts that the pinned tiling really runs exactly there and checks every one
of those layers bit for bit (check_exact of test_layer_exact_gpu.py: output, per-channel sum, sum of squares; Winograd F(4x4,3x3) inside
its componentwise bound).  A new menu entry is therefore tested without anyone writing its name down; a menu that outgrows MENU_SLOTS or
an entry that is legal nowhere fails test_menu_cpu.py.

  test_exact_menu_slot[i]            the six fp32 menus (3x3 stride 1 / 2, the three upsamplers, the head)
  test_exact_g1x1_16bit_slot[mode,i] the two gemm1x1 tilings of the upsamplers and the head in each 16-bit mode
  (conv16's menus: test_layer_exact_gpu.test_exact_conv16_forced_shape, whose shape list test_menu_cpu.py proves complete)
  test_exact_head_cls[pd]            the three ring depths of the cls-only head pass, on both head images it can read
  test_exact_strip_tilings           the four strip tilings of wino4 / wino6, and the rounded-up masked form of the same map
The tests do not switch the tuner off: PP_FORCE_VARIANT is read by the measuring path only.  Layers outside the pinned kinds are tuned
once per process and cached."""
import ctypes
import time

import numpy as np
import pytest
import torch

import layer_ref as R
import menu_cases as M
from test_layer_exact_gpu import FORCED_COMBOS, check_exact, dev, exact_sd, host, make_engine, tally  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

G1X1_KEYS = ("up1", "up2", "up4", "head")


def run_slot(mode, i, keys, synth, sd, tally, monkeypatch):
    """Pin entry i of the menus `keys` of `mode`, build one engine per grid, check that the pinned tilings run exactly the layers the CPU
    table calls legal, and run each of them through check_exact.  Returns {name: layers run}."""
    names = M.slot_names(mode, i, keys)
    if not names:
        print(f"[menu slot] {mode} slot {i}: beyond every menu's length, nothing to pin")
        return {}
    monkeypatch.setenv("PP_FORCE_VARIANT", ";".join(names.values()))
    expect = M.slot_layers(mode, i, R.GRIDS, keys)
    ran = {name: 0 for name in names.values()}
    t0 = time.time()
    for grid in sorted(R.GRIDS):
        eng = make_engine(synth, grid, mode, sd)
        til = eng.layer_tilings()
        shapes = R.plan_shapes(*R.GRIDS[grid])
        for index, t in enumerate(til):
            want = expect.get((grid, index))
            key = M.menu_key(shapes[index], index, mode)
            if want is not None:  # legal by the CPU table: the layer carries the pinned name ...
                assert t["tiling"] == want, (grid, index, t["tiling"], want)
            elif key in names:    # ... illegal: it cannot (the tuner chose among the legal entries)
                assert t["tiling"] != names[key], (grid, index, t["tiling"], "runs a layer the table calls illegal")
            if want is None:
                continue
            for pre, with_res in FORCED_COMBOS:
                if with_res and t["kind"] != 0:
                    continue
                assert check_exact(eng, sd, index, grid, pre, with_res, tally, mode) == want
            ran[want] += 1
        del eng
    never = {n for (m, key, n) in M.NEVER_LEGAL if m == mode}
    for name, n in ran.items():
        assert n > 0 or name in never, f"{name} ran on no layer"
    print(f"[menu slot] {mode} slot {i}: " + ", ".join(f"{name} x{n}" for name, n in ran.items()) + f" ({time.time() - t0:.1f} s)")
    return ran


@pytest.mark.parametrize("i", range(M.MENU_SLOTS))
def test_exact_menu_slot(i, synth, exact_sd, tally, monkeypatch):
    """Entry i of every fp32 menu.  Level 0's stride-1 layers run the roofline-tagged instantiation of a Winograd tiling, the other
    levels the plain one; both grids have all three levels."""
    ran = run_slot("fp32", i, None, synth, exact_sd, tally, monkeypatch)
    longest = max(len(rows) for rows in M.legal_table("fp32").values())
    assert bool(ran) == (i < longest)


@pytest.mark.parametrize("i", (0, 1))
@pytest.mark.parametrize("mode", R.MODES[1:])
def test_exact_g1x1_16bit_slot(mode, i, synth, exact_sd, tally, monkeypatch):
    """Both gemm1x1 tilings of the three upsamplers and the head in every 16-bit mode (fp16s: on fp16 tensors)."""
    ran = run_slot(mode, i, G1X1_KEYS, synth, exact_sd, tally, monkeypatch)
    assert len(ran) == 4 and all(n.startswith("g1x1") and n.split()[-1] == f"p{3 if mode == 'fp16s' else R.MODES.index(mode)}" for n in ran)
    assert all(n >= 2 for n in ran.values()), ran  # each on both grids


def head_case(sd, grid, pre):
    c = R.exact_case(sd, 19, grid, pre, False)
    return c, dict(x=dev(c["x"]), scale=dev(c["scale"]), shift=dev(c["shift"]))


@pytest.mark.parametrize("pd", ["pd8", "pd10", "pd4"])
def test_exact_head_cls(pd, synth, exact_sd, monkeypatch):
    """The cls-only pass of the deferred head at each ring depth: bit-equal to the cls part of the reference and to the full head's cls
    output, three frames, shared and per-frame prologue.  The pass gathers its 16-row slab out of the head's committed image, whose
    layout depends on the head's own tiling, so each ring depth runs on both gemm1x1 head images; the head's name follows the cls name
    in PP_FORCE_VARIANT ("a;b": every menu takes the first of the two it has), which also keeps the tuner from moving the head of these
    small maps onto a direct tiling, where there is no deferred head.  The small maps have fewer work items than persistent workgroups."""
    eng_mod = M.engine_mod()
    cls_names = [n for n in eng_mod.menu_names(which="cls") if f" {pd} " in n]
    assert len(cls_names) == 1
    heads = [n for n, _ in M.legal_table("fp32")["head"] if n.startswith("g1x1")]
    assert len(heads) == 2
    for head_name in heads:
        monkeypatch.setenv("PP_FORCE_VARIANT", f"g1x1 cls {pd};{head_name}")
        for grid in sorted(R.GRIDS):
            eng = make_engine(synth, grid, "fp32", exact_sd)
            assert eng.head_cls_tiling() == cls_names[0] and eng.layer_tilings()[19]["tiling"] == head_name
            for pre in ("shared", "frame"):
                c, args = head_case(exact_sd, grid, pre)
                cls = eng.debug_head_cls(**args)
                full = eng.debug_layer(19, **args)
                torch.cuda.synchronize()
                assert cls.shape == (R.NB, eng.A, 1)
                assert np.array_equal(host(cls), c["ref"][0].astype(np.float32)), (pd, head_name, grid, pre)
                assert torch.equal(cls, full[0]), (pd, head_name, grid, pre)
            del eng
    print(f"[menu] cls-only pass {cls_names[0]}: bit-exact on {len(heads)} head images x {len(R.GRIDS)} grids x 2 prologues")


def test_head_cls_hook_refuses_what_it_cannot_run(synth, exact_sd, monkeypatch):
    """No deferred head in a 16-bit plan: the hook raises and launches nothing; bad arguments on a plan that has one likewise."""
    grid = "64x96"
    c, args = head_case(exact_sd, grid, "shared")
    monkeypatch.setenv("PP_FORCE_VARIANT", M.legal_table("fp32")["head"][0][0])  # the head on gemm1x1 in both plans
    eng = make_engine(synth, grid, "fp16", exact_sd)
    assert eng.head_cls_tiling() == "" and eng.layer_tilings()[19]["tiling"].startswith("g1x1")
    with pytest.raises(RuntimeError, match="no deferred head"):
        eng.debug_head_cls(**args)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    out = torch.full((R.NB, eng.A), 7.0, device="cuda")
    x, sc, sh = p(args["x"]), p(args["scale"]), p(args["shift"])
    assert eng.lib.pp_debug_head_cls(eng.ctx, R.NB, x, 1, sc, sh, p(out), None) != 0
    assert eng.lib.pp_last_error(eng.ctx)
    del eng
    eng = make_engine(synth, grid, "fp32", exact_sd)
    assert eng.head_cls_tiling().startswith("g1x1 cls pd")
    for a in ((0, x, 1, sc, sh, p(out)), (R.NB + 1, x, 1, sc, sh, p(out)), (R.NB, None, 1, sc, sh, p(out)), (R.NB, x, 1, sc, sh, None),
              (R.NB, x, 3, sc, sh, p(out)), (R.NB, x, 1, sc, None, p(out)), (R.NB, x, 0, sc, sh, p(out))):
        assert eng.lib.pp_debug_head_cls(eng.ctx, *a, None) != 0, a
        assert eng.lib.pp_last_error(eng.ctx)
    for bad in (lambda: eng.debug_head_cls(args["x"][:, :-1]), lambda: eng.debug_head_cls(args["x"], scale=args["scale"]),
                lambda: eng.debug_head_cls(torch.cat([args["x"], args["x"]])), lambda: eng.debug_head_cls(args["x"].cpu())):
        with pytest.raises((ValueError, TypeError)):
            bad()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    good = eng.debug_head_cls(**args)  # the next valid call works
    torch.cuda.synchronize()
    assert np.array_equal(host(good), c["ref"][0].astype(np.float32))


@pytest.mark.parametrize("strips", ["2", "0"])
@pytest.mark.parametrize("family", ["wino4 tw4 bx2", "wino6 tw4"])
def test_exact_strip_tilings(family, strips, synth, exact_sd, tally, monkeypatch):
    """The 36 x 44 level-0 map of the strip grid: 2 x 2 main tiles + a right strip of 4 x 64 px tiles (12 px wide) + a bottom strip of
    64 x 4 px tiles (4 px tall) with PP_W4_STRIPS=2, 3 x 3 rounded-up main tiles with masked lanes with PP_W4_STRIPS=0 -- each level-0
    stride-1 layer as a single exact layer, per-frame prologue, with and without residual.  wino4 bit for bit, wino6 inside
    winograd4_bound (check_exact)."""
    grid = next(iter(R.STRIP_GRID))
    monkeypatch.setenv("PP_FORCE_VARIANT", family)
    monkeypatch.setenv("PP_W4_STRIPS", strips)
    eng = make_engine(synth, grid, "fp32", exact_sd)
    til = eng.layer_tilings()
    layers = [k for k, t in enumerate(til) if t["kind"] == 0 and t["stride"] == 1 and t["level"] == 0 and family in t["tiling"]]
    want = sorted(k for n, where in M.legal_table("fp32")["k3s1"] for g, k in where if g == grid and family in n and til[k]["level"] == 0)
    assert layers == want == [1, 2, 3], (layers, want, til[1:4])
    assert (eng.H, eng.W) == (36, 44)
    for k in layers:
        for with_res in (False, True):
            assert family in check_exact(eng, exact_sd, k, grid, "frame", with_res, tally, "fp32")
    print(f"[menu] {family} on 36 x 44, PP_W4_STRIPS={strips}: {len(layers)} layers x 2 cases " + ("inside the F(4x4) bound" if "wino6" in family else "bit-exact"))
