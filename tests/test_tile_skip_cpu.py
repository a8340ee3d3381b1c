"""CPU (-m "not gpu"): the numpy restatement of the tile-skipping rule (tests/tile_skip_ref.py) on hand-made maps, and the skip
fractions it gives on the benchmark's own cloud."""
import numpy as np
import pytest

import tile_skip_ref as T

H, W = 64, 80  # 4 x 5 tiles: every class exists, 6 interior tiles
NTY, NTX = H // 16, W // 16


def flags_of(pixels):
    act = np.zeros((H, W), bool)
    for y, x in pixels:
        act[y, x] = True
    return T.tile_flags(act)


def test_empty_map_everything_skippable_one_item_per_class():
    f = flags_of([])
    assert f.shape == (3, NTY, NTX) and f.all()
    for k in range(3):
        items, fills = T.lists(f[k])
        assert len(items) == 9 and len(fills) == NTY * NTX - 9
        assert sum(m for _, m in items) == NTY * NTX  # the statistics count every tile once
        assert dict(items)[6] == 6   # first interior tile (1, 1) stands for the 6 interior tiles
        for dst, src in fills:
            assert src < dst and T.tile_class(dst // NTX, dst % NTX, NTY, NTX) == T.tile_class(src // NTX, src % NTX, NTY, NTX)
        items_i, fills_i = T.lists(f[k], border=False)
        assert len(items_i) == NTY * NTX - 5 and len(fills_i) == 5


def test_one_pixel_at_a_tile_centre():
    f = flags_of([(24, 40)])  # centre of tile (1, 2): blocks (5..6, 9..10) see it; the tile spans blocks 4..7 x 8..11
    want = np.ones((NTY, NTX), bool)
    want[1, 2] = False
    assert np.array_equal(f[0], want)
    assert np.array_equal(f[1], want)  # one dilation: blocks 4..7 x 8..11, still inside the tile
    want3 = np.ones((NTY, NTX), bool)
    want3[0:3, 1:4] = False            # two dilations: blocks 3..8 x 7..12 reach the eight neighbours
    assert np.array_equal(f[2], want3)


def test_one_pixel_on_a_four_tile_junction():
    f = flags_of([(16, 16)])  # first pixel of tile (1, 1): the 6x6 windows of blocks (3..4, 3..4) hold it
    want = np.ones((NTY, NTX), bool)
    want[0:2, 0:2] = False
    for k in range(3):
        assert np.array_equal(f[k], want)  # dilations stay inside the four tiles (blocks 1..6)


def test_pixels_at_the_corners():
    f = flags_of([(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)])
    want = np.ones((NTY, NTX), bool)
    for ty in (0, NTY - 1):
        for tx in (0, NTX - 1):
            want[ty, tx] = False
    for k in range(3):
        assert np.array_equal(f[k], want)
    items, fills = T.lists(f[0])
    # the four corner classes have no skippable tile: computed with mult 1; edges and interior keep one representative each
    assert sorted(m for _, m in items) == [1, 1, 1, 1, 2, 2, 3, 3, 6]


def test_full_border():
    px = [(y, x) for y in range(H) for x in range(W) if y in (0, H - 1) or x in (0, W - 1)]
    f = flags_of(px)
    want = np.zeros((NTY, NTX), bool)
    want[1:-1, 1:-1] = True
    for k in range(3):
        assert np.array_equal(f[k], want)  # the border's influence ends 3 blocks in: less than a tile
    items, fills = T.lists(f[2])
    assert len(fills) == 5 and sum(m for _, m in items) == NTY * NTX


def test_full_map_nothing_skippable():
    f = T.tile_flags(np.ones((H, W), bool))
    assert not f.any()
    items, fills = T.lists(f[0])
    assert items == [(t, 1) for t in range(NTY * NTX)] and fills == []


def test_blocks_window_is_six_by_six():
    act = np.zeros((H, W), bool)
    act[19, 20] = True  # last row of block row 4, first column of block column 5
    b = T.blocks(act)
    want = np.zeros_like(b)
    want[4:6, 4:6] = True  # the windows of rows 4, 5 (pixels 15..20, 19..24) and columns 4, 5 (15..20, 19..24)
    assert np.array_equal(b, want)


def test_skip_fractions_of_the_benchmark_cloud(synth):
    """synth.lidar_cloud("eight_20cm", seed=1000), the first cloud bench.py feeds: share of the 625 level-0 tiles that are skippable at
    layers 1, 2, 3, with border tiles."""
    from oracle import c_oracle as C
    from oracle import pp_oracle as O
    cfg = synth.load_config("eight_20cm")
    s = O.voxel_setup(cfg)
    pts = synth.lidar_cloud("eight_20cm", seed=1000)
    _, coors, _ = C.points_to_voxels(pts, s["voxel_size"], s["offset"], s["grid_size"], cfg["max_voxels"], cfg["max_num_points"])
    gx, gy = int(s["grid_size"][0]), int(s["grid_size"][1])
    assert (gx, gy) == (800, 800)
    act = T.active_from_coors(coors[:, :2], gx, gy)
    f = T.tile_flags(act)
    frac = [T.skip_fraction(f[k]) for k in range(3)]
    inner = [T.skip_fraction(f[k], border=False) for k in range(3)]
    print(f"[tile skip] seed 1000: active {act.mean():.4f}, skippable with border {frac}, interior only {inner}")
    assert [round(x, 3) for x in frac] == [0.515, 0.379, 0.312]
    assert all(i < b for i, b in zip(inner, frac))
