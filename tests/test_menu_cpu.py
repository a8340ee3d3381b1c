"""CPU (-m "not gpu"): the tuner's menus, read from the library without a device (engine.menu_names -> pp_menu_names), against what the
slot tests of test_menu_exact_gpu.py rely on: no menu longer than MENU_SLOTS, names that PP_FORCE_VARIANT's substring matching can tell
apart, and every entry legal on some layer of the test grids -- or listed in menu_cases.NEVER_LEGAL with its reason."""
import pytest

import layer_ref as R
import menu_cases as M
from conftest import load_pkg

# every way layer_menu can be asked for a menu: (kind, stride, up, cin), cin both with and without the factors the menus look at
CONVS = [(0, s, 1, cin) for s in (1, 2) for cin in (64, 128, 256, 48, 24)]
UPS = [(1, 1, up, cin) for up in (1, 2, 4) for cin in (64, 128, 256, 48)]
HEADS = [(2, 1, 1, cin) for cin in (320, 48)]


def all_menus():
    eng = load_pkg("engine")
    for mode in R.MODES:
        for kind, stride, up, cin in CONVS + UPS + HEADS:
            for head9 in (True, False):
                for first in ((False, True) if (kind, stride) == (0, 2) else (False,)):
                    yield (mode, kind, stride, up, cin, head9, first), eng.menu_names(kind=kind, stride=stride, up=up, cin=cin, precision=mode,
                                                                                     head9=head9, first_conv=first)
    yield ("cls",), eng.menu_names(which="cls")
    yield ("strips",), eng.menu_names(which="strips")


def test_menus_fit_the_slots_and_are_not_empty():
    longest, n = 0, 0
    for what, menu in all_menus():
        assert 0 < len(menu) <= M.MENU_SLOTS, (what, len(menu))
        longest, n = max(longest, len(menu)), n + 1
    assert n > 200
    print(f"[menu] {n} menus, the longest has {longest} of {M.MENU_SLOTS} entries")


def test_names_are_unique_and_no_name_contains_another():
    """PP_FORCE_VARIANT takes the first entry a name is a substring of: a full name must select its own entry and nothing else."""
    for what, menu in all_menus():
        if what == ("strips",):  # not selectable by name: they follow the main tile's family
            assert len(set(menu)) == len(menu)
            continue
        for i, a in enumerate(menu):
            for j, b in enumerate(menu):
                assert i == j or a not in b, (what, a, b)


def test_menus_of_different_layer_kinds_share_no_name():
    """One engine pins one entry per layer kind: a name forced for one kind must not match an entry of another kind's menu (nor the
    cls-only menu, which reads PP_FORCE_VARIANT too)."""
    for mode in R.MODES:
        table = M.legal_table(mode)
        names = {key: [n for n, _ in rows] for key, rows in table.items()}
        names["cls"] = load_pkg("engine").menu_names(which="cls")
        for ka, a in names.items():
            for kb, b in names.items():
                if ka != kb:
                    assert not [(x, y) for x in a for y in b if x in y], (mode, ka, kb)


def test_menu_names_takes_the_plan_arguments_and_the_buffer_convention():
    eng = load_pkg("engine")
    lib = load_pkg("_lib").load()
    import ctypes
    args = (0, 0, 1, 1, 64, 0, 1, 0, 0, 0, 0, 0)
    n = lib.pp_menu_names(*args, None, 0)
    full = ctypes.create_string_buffer(n + 1)
    assert lib.pp_menu_names(*args, full, n + 1) == n and len(full.value) == n and full.value.endswith(b"\n")
    short = ctypes.create_string_buffer(b"#" * 16, 16)
    assert lib.pp_menu_names(*args, short, 8) == n and short.raw[:8] == full.value[:7] + b"\0" and short.raw[8:] == b"#" * 8
    for bad in ((3,) + args[1:], (0, 3) + args[2:], (0, 0, 3) + args[3:], (0, 1, 1, 3) + args[4:], args[:5] + (5,) + args[6:]):
        assert lib.pp_menu_names(*bad, None, 0) < 0, bad
    with pytest.raises(ValueError):
        eng.menu_names(kind=0, stride=3)
    # the precision by name or number; the shape form is a subsequence of the menu, in menu order
    assert eng.menu_names(kind=0, stride=1, cin=64, precision="bf16") == eng.menu_names(kind=0, stride=1, cin=64, precision=2)
    menu = eng.menu_names(kind=0, stride=1, cin=64)
    some = eng.menu_names(kind=0, stride=1, cin=64, shape=(64, 9, 11, 11))
    assert some and len(some) < len(menu) and some == [n for n in menu if n in some]
    assert not [n for n in some if n.startswith(("wino4", "wino6"))]  # an odd map: no float2 rows, no whole 4x4 tiles
    # what the menus look at: a head of other than 9 anchors and Cin off the 32 / 16 grid lose the persistent GEMM / the 16-bit kernels
    assert not [n for n in eng.menu_names(kind=2, cin=320, head9=False) if n.startswith("g1x1")]
    assert not [n for n in eng.menu_names(kind=1, up=2, cin=48) if n.startswith("g1x1")]
    assert all(n.startswith("c16") for n in eng.menu_names(kind=0, stride=1, cin=48, precision="fp16"))
    assert not [n for n in eng.menu_names(kind=0, stride=1, cin=24, precision="fp16") if n.startswith("c16")]
    assert [n for n in eng.menu_names(kind=0, stride=1, cin=64) if n.startswith("wino6")] and not [n for n in eng.menu_names(kind=0, stride=1, cin=48) if n.startswith("wino6")]


def test_the_plan_reaches_one_menu_per_kind():
    """All layers of a kind share one menu whatever their level and Cin (legal_table asserts it while it builds), and the keys are the
    six kinds -- plus the first conv's own menu in fp16s."""
    for mode in R.MODES:
        keys = set(M.legal_table(mode))
        assert keys == {"k3s1", "k3s2", "up1", "up2", "up4", "head"} | ({"k3s2 first"} if mode == "fp16s" else set()), (mode, keys)
        if mode != "fp32":  # the reduced modes run their own kernels everywhere: conv16 and the PREC instantiations of gemm1x1
            tag = f"p{3 if mode == 'fp16s' else R.MODES.index(mode)}"
            for key, rows in M.legal_table(mode).items():
                assert all(n.startswith("c16" if key.startswith("k3") else "g1x1") and tag in n.split() for n, _ in rows), (mode, key)


@pytest.mark.parametrize("mode", R.MODES)
def test_every_entry_is_legal_on_a_test_grid_or_listed(mode):
    """Every entry of every menu a 9-anchor plan can reach is legal on at least one layer of the grids the slot tests build their
    engines on (R.GRIDS) -- so pinning it runs it -- unless NEVER_LEGAL lists it."""
    table = M.legal_table(mode)
    never = {(key, name) for (m, key, name) in M.NEVER_LEGAL if m == mode}
    seen = set()
    for key, rows in table.items():
        for name, where in rows:
            on_slot_grids = [(g, k) for g, k in where if g in R.GRIDS]
            if (key, name) in never:
                assert not where, (mode, key, name, "is legal after all: take it out of NEVER_LEGAL", where)
                seen.add((key, name))
            else:
                assert on_slot_grids, (mode, key, name, "is legal on no layer of R.GRIDS: the slot tests cannot run it")
            for g, k in where:
                L = R.plan_shapes(*R.ALL_GRIDS[g])[k]
                assert M.menu_key(L, k, mode) == key
    assert seen == never, never - seen  # no stale line in NEVER_LEGAL
    n = sum(len(rows) for rows in table.values())
    print(f"[menu] {mode}: {n} entries in {len(table)} menus, {len(never)} never legal")


def test_never_legal_entries_are_dead_at_full_size_too(synth):
    """An entry no test grid can run must be one that no shipped configuration can run either -- otherwise the grids have a gap."""
    eng = load_pkg("engine")
    for name in ("eight_20cm", "ntusl_10cm", "nuscene", "nuscene_10class"):
        grid = eng.snap_geometry(synth.load_config(name))[2]
        gx, gy = int(grid[0]), int(grid[1])
        for mode in R.MODES:
            dead = {(key, n) for (m, key, n) in M.NEVER_LEGAL if m == mode}
            for index, L in enumerate(R.plan_shapes(gx, gy)):
                legal = M.layer_menu(L, index, mode, shape=True)
                assert legal, (name, mode, index)  # the full-size maps take every mode
                hit = [n for n in legal if (M.menu_key(L, index, mode), n) in dead]
                assert not hit, (name, mode, index, hit)
    assert all(reason for reason in M.NEVER_LEGAL.values())


def test_hand_written_force_lists_still_resolve():
    """The substrings the older tests pin (FP32_FORCED, C16_SHAPES) each match an entry, and -- the other way round -- every conv16 entry
    of every 16-bit mode carries one of the C16_SHAPES, so test_exact_conv16_forced_shape enumerates conv16's menus completely."""
    import ast
    import os

    def constant(path, name):  # the lists live in GPU test modules: read them without importing torch-on-device code
        tree = ast.parse(open(os.path.join(os.path.dirname(__file__), path)).read())
        for node in tree.body:
            if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in node.targets):
                return ast.literal_eval(node.value)
        raise KeyError(name)

    fp32_forced, c16_shapes = constant("test_layer_exact_gpu.py", "FP32_FORCED"), constant("test_gpu_parity.py", "C16_SHAPES")
    assert len(fp32_forced) >= 13 and len(c16_shapes) == 13
    fp32 = [n for rows in M.legal_table("fp32").values() for n, _ in rows]
    for force in fp32_forced:
        assert [n for n in fp32 if force in n], force
    for mode in R.MODES[1:]:
        conv16 = [n for key, rows in M.legal_table(mode).items() if key.startswith("k3") for n, _ in rows]
        assert len(conv16) == (23 if mode == "fp16s" else 17)
        for shape in c16_shapes:
            assert [n for n in conv16 if shape in n], (mode, shape)
        for n in conv16:
            assert sum(shape in n for shape in c16_shapes) == 1, (mode, n)


def test_strip_grid_is_what_the_strip_test_needs():
    gx, gy = R.STRIP_GRID["72x88"]
    L = R.plan_shapes(gx, gy)[1]
    assert (L["h"], L["w"]) == (36, 44) and L["h"] // 16 == 2 and L["w"] // 16 == 2 and L["w"] % 16 == 12 and L["h"] % 16 == 4
    assert "72x88" not in R.GRIDS and set(R.ALL_GRIDS) == set(R.GRIDS) | {"72x88"}
    table = M.legal_table("fp32")["k3s1"]
    for family in ("wino4 tw4 bx2", "wino6 tw4"):  # the main tiles whose strips the test runs are legal on the three level-0 layers
        hits = [where for n, where in table if family in n]
        assert len(hits) == 1 and {k for g, k in hits[0] if g == "72x88"} >= {1, 2, 3}, family
    strips = load_pkg("engine").menu_names(which="strips")
    assert len(strips) == 4 and [s.split()[0] for s in strips] == ["wino4", "wino4", "wino6", "wino6"]
    assert load_pkg("engine").menu_names(which="strips", cin=64, shape=(64, 36, 44, 44)) == strips
