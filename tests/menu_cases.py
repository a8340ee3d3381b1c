"""The tuner's menus as the library reports them (engine.menu_names -> pp_menu_names; no device needed) and, for every entry, the
(grid, layer) pairs of the test grids on which the library calls it legal.  test_menu_cpu.py checks this table, test_menu_exact_gpu.py
takes it as its expectation: the tiling pinned for slot i must really run every layer the table lists for it.  Nothing here names a
tiling except NEVER_LEGAL."""
import layer_ref as R
from conftest import load_pkg

MENU_SLOTS = 32  # no menu may be longer: test_menu_exact_gpu parametrises test_exact_menu_slot over range(MENU_SLOTS)
HEAD_ROWS = 96   # GEMM rows of the 9-anchor head (90 padded to the 96-row block of its tilings)

# Menu entries that are legal on no layer of any grid, with the reason.  A finding, not a licence: test_menu_cpu asserts that each is
# illegal on every layer of the four shipped configurations at full size too, i.e. that it is dead weight of the menu, not a gap of the
# test grids.  Key: (mode, menu key, name).
_UP1_128 = ("the up = 1 upsampler has 64 GEMM rows (64 output channels x 1 x 1) and a direct tiling must not be taller than its rows rounded up to 64: "
            "the 128-row tilings of conv_menu can never run it")
NEVER_LEGAL = {("fp32", "up1", name): _UP1_128 for name in (
    "k1s1 tw8 w2x2 t4x5 bx5 kc16 e0", "k1s1 tw8 w2x2 t4x5 bx5 kc8 e0", "k1s1 tw8 w4x1 t2x5 bx5 kc16 e0", "k1s1 tw8 w2x2 t4x2 bx2 kc16 e0",
    "k1s1 tw4 w4x1 t2x5 bx5 kc16 e0", "k1s1 tw4 w4x1 t2x5 bx5 kc8 e0", "k1s1 tw4 w8x1 t1x5 bx5 kc16 e0", "k1s1 tw4 w2x2 t4x5 bx5 kc16 e0",
    "k1s1 tw4 w2x2 t4x2 bx2 kc16 e0")}
_FIRST_128 = ("fp16s gives the first conv (64 output channels) the stride-2 conv16 menu with an fp32 input tensor (h2) as a menu of its own, and "
              "conv16 tiles whole row blocks: its three 128-row shapes can never run the only layer that menu serves")
NEVER_LEGAL.update({("fp16s", "k3s2 first", name): _FIRST_128 for name in (
    "c16 s2 p3 h2 w4x1 t1x5 20x8 o2", "c16 s2 p3 h2 w4x2 t1x5 40x8 o2", "c16 s2 p3 h2 w4x1 t1x5 20x8 o1")})


def engine_mod():
    return load_pkg("engine")


def menu_key(L, index, mode):
    """Which menu layer `index` (a plan_shapes entry) chooses from.  fp16s gives the first conv a menu of its own (fp32 input tensor)."""
    if L["kind"] == 2:
        return "head"
    if L["kind"] == 1:
        return f"up{L['up']}"
    return f"k3s{L['stride']}" + (" first" if mode == "fp16s" and index == 0 else "")


def layer_rows(L):
    return HEAD_ROWS if L["kind"] == 2 else L["cout"] * L["up"] * L["up"]


def layer_menu(L, index, mode, shape=False):
    """The menu of plan layer `index` in `mode`, named the way the plan composes it; shape=True: only the entries legal on the layer's maps."""
    return engine_mod().menu_names(kind=L["kind"], stride=L["stride"], up=L["up"], cin=L["cin"], precision=mode, head9=True, first_conv=index == 0,
                                   shape=(layer_rows(L), L["hin"], L["win"], L["w"]) if shape else None)


_TABLES = {}


def legal_table(mode):
    """{menu key: [(name, [(grid, layer index), ...]), ...] in menu order} over the layers of a 9-anchor plan on R.ALL_GRIDS.  A layer
    none of whose mode entries is legal falls back to its fp32 menu in the plan; it is then simply in no list of the mode's table."""
    if mode in _TABLES:
        return _TABLES[mode]
    table = {}
    for grid in sorted(R.ALL_GRIDS):
        for index, L in enumerate(R.plan_shapes(*R.ALL_GRIDS[grid])):
            key, menu = menu_key(L, index, mode), layer_menu(L, index, mode)
            rows = table.setdefault(key, [(name, []) for name in menu])
            assert [name for name, _ in rows] == menu, (mode, key, grid, index)  # one menu per key, whatever the level
            legal = set(layer_menu(L, index, mode, shape=True))
            assert legal <= set(menu)
            for name, where in rows:
                if name in legal:
                    where.append((grid, index))
    _TABLES[mode] = table
    return table


def slot_names(mode, i, keys=None):
    """{menu key: name of entry i} for the menus of `mode` that have an entry i"""
    return {key: rows[i][0] for key, rows in legal_table(mode).items() if (keys is None or key in keys) and i < len(rows)}


def slot_layers(mode, i, grids, keys=None):
    """{(grid, layer index): name} -- every layer on `grids` that entry i of its menu is legal for"""
    out = {}
    for key, rows in legal_table(mode).items():
        if (keys is None or key in keys) and i < len(rows):
            out.update({(g, k): rows[i][0] for g, k in rows[i][1] if g in grids})
    return out
