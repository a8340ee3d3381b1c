"""Tile skipping in the stride-1 layers of level 0 (-m gpu): behind the sparse first conv, the fp32 wino6 launches compute one 16 x 16
tile per (frame, layer, border class) of those whose input is constant, weight its statistics by the class's count and copy it to the
others (csrc/tile_skip.hip).  Checked on a 128 x 160-cell grid -- level-0 map 64 x 80 = 4 x 5 tiles: every border
class exists, each edge class has at least two tiles, six interior tiles -- with the wino6 tiling pinned: the tile flags against the
numpy rule (tests/tile_skip_ref.py), single layers bit for bit against their dense launch, the whole pass switch on against switch
off, independence of a frame from its batch, and the fallback on a map that is not a whole number of tiles."""
import os

import numpy as np
import pytest
import torch

import layer_ref as R
import tile_skip_ref as T
from conftest import load_pkg
from frame_check import report

pytestmark = pytest.mark.gpu

GX, GY, H, W = 128, 160, 64, 80
NTY, NTX = H // 16, W // 16
OVER = dict(detection_range=[0.0, 0.0, -2.5, 0.2 * GX, 0.2 * GY, 8.5], max_voxels=GX * GY)
MAXB = 34  # crosses PP_GROUP = 32


def make_cfg(synth, **over):
    cfg = synth.load_config("eight_20cm")
    cfg.update(OVER)
    cfg.update(over)
    cfg["device"] = torch.device("cuda:0")
    return cfg


def cloud_of_cells(cells, y0=0.0):
    """One point in the centre of every (cx, cy) cell."""
    c = np.asarray(cells, np.float32).reshape(-1, 2)
    pts = np.zeros((c.shape[0], 4), np.float32)
    pts[:, 0] = (c[:, 0] + 0.5) * 0.2
    pts[:, 1] = y0 + (c[:, 1] + 0.5) * 0.2
    pts[:, 2] = 0.5
    pts[:, 3] = 0.3
    return pts


BORDER = [(x, y) for x in range(GX) for y in range(GY) if x in (0, GX - 1) or y in (0, GY - 1)]
FRAMES = {
    "none": np.array([[-5.0, 0.0, 0.0, 0.1]], np.float32),       # the only point lies outside the range
    "centre": cloud_of_cells([(GX // 2, GY // 2)]),              # even cell: output pixel (32, 40) alone, the middle of tile (2, 2)
    "corner": cloud_of_cells([(0, 0)]),
    "border": cloud_of_cells(BORDER),
    "junction": cloud_of_cells([(32, 32)]),                      # output pixel (16, 16): the first pixel of tile (1, 1)
    "full": cloud_of_cells([(x, y) for x in range(GX) for y in range(GY)]),
}


def forced_engine(synth, cfg, max_batch):
    old = os.environ.get("PP_FORCE_VARIANT")
    os.environ["PP_FORCE_VARIANT"] = "wino6"
    try:
        e = load_pkg("engine").Engine(cfg, max_batch=max_batch)
        e.load_state_dict(synth.seeded_state_dict(6, cls_bias=-3.0))
    finally:
        if old is None:
            del os.environ["PP_FORCE_VARIANT"]
        else:
            os.environ["PP_FORCE_VARIANT"] = old
    return e


@pytest.fixture(scope="module")
def eng(synth):
    e = forced_engine(synth, make_cfg(synth), MAXB)
    assert (e.H, e.W) == (H, W)
    til = e.layer_tilings()
    assert all(til[i]["wino"] == 6 and til[i]["level"] == 0 and til[i]["stride"] == 1 for i in (1, 2, 3))
    return e


@pytest.fixture(scope="module")
def clouds(synth):
    d = dict(FRAMES)
    d["lidar"] = synth.lidar_cloud("eight_20cm", seed=5)  # cropped to the grid by the voxeliser
    return d


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def reference_flags(eng, frame):
    n = int(eng.fetch(frame, "num").cpu().numpy()[0])
    coors = eng.fetch(frame, "coors").cpu().numpy()[:n]
    return n, T.tile_flags(T.active_from_coors(coors[:, :2], GX, GY))


@pytest.mark.parametrize("name", list(FRAMES) + ["lidar"])
def test_tile_flags_against_the_rule(eng, clouds, name):
    eng.set_sparse_conv1(True)
    eng.set_tile_skip(True)
    eng.infer_frame(dev(clouds[name]))
    torch.cuda.synchronize()
    assert eng.tile_skip_active()
    got = eng.fetch(0, "tile_flags").cpu().numpy().astype(bool)
    n, want = reference_flags(eng, 0)
    print(f"[tile skip] {name}: {n} pillars, skippable tiles of {NTY * NTX} at layers 1..3: {[int(want[k].sum()) for k in range(3)]}")
    assert got.shape == want.shape == (3, NTY, NTX)
    assert np.array_equal(got, want)
    if name == "none":
        assert want.all()
    if name == "full":
        assert not want.any()
    if name == "lidar":
        assert n > 300


def test_single_layers_bit_for_bit(eng):
    """Layers 1, 2, 3 through the hook, three frames (empty / one pixel / full), per-frame prologue, dyadic inputs: the listed launch
    plus fill against the dense launch of the same layer on the same tensors.  Input and residual of layers 2 and 3 are the previous
    layers' outputs, so they satisfy the rule's precondition: constant per channel outside the non-constant blocks."""
    eng.set_tile_skip(True)
    rng = np.random.default_rng(11)
    act = np.zeros((3, H, W), bool)
    act[1, 24, 40] = True
    act[2] = True
    # what the norm + ReLU in front of the first unit leaves: dyadic values on the active pixels, one constant per channel elsewhere
    const = rng.integers(0, 8, (3, 64, 1, 1)).astype(np.float32) * 0.25
    x0 = np.where(act[:, None], R.exact_activations(rng, (3, 64, H, W)).astype(np.float32), const).astype(np.float32)
    bitmap = dev(act.astype(np.uint8))
    aff = [tuple(dev(a) for a in R.exact_affine(rng, (3, 64))) for _ in range(3)]
    x0d = dev(x0)
    ins = {1: (x0d, None)}
    for k in (1, 2, 3):
        x, res = ins[k]
        sc, sh = aff[k - 1]
        dense, st_d = eng.debug_layer(k, x=x, res=res, scale=sc, shift=sh, stats=True)
        torch.cuda.synchronize()
        assert not eng.tile_skip_active()
        listed, st_l = eng.debug_layer(k, x=x, res=res, scale=sc, shift=sh, stats=True, active=bitmap, skip_k=k)
        torch.cuda.synchronize()
        assert eng.tile_skip_active()
        d, l = dense.cpu().numpy(), listed.cpu().numpy()
        sd_, sl_ = st_d.cpu().numpy(), st_l.cpu().numpy()
        rel = float((np.abs(sd_ - sl_) / np.maximum(np.maximum(np.abs(sd_), np.abs(sl_)), 1e-300)).max())
        nskip = [int(T.tile_flags(act[f])[k - 1].sum()) for f in range(3)]
        print(f"[tile skip] layer {k}: skippable tiles per frame {nskip}, outputs equal {np.array_equal(d, l)}, statistics max relative difference {rel:.2e}")
        assert np.isfinite(d).all()
        assert np.array_equal(d, l), (k, float(np.abs(d - l).max()))
        assert rel <= 1e-12, (k, rel)
        assert nskip[0] == NTY * NTX and nskip[2] == 0
        if k == 1:
            ins[2] = (dense, x0d)
        elif k == 2:
            ins[3] = (dense, dense)


def tensors(eng, pts):
    eng.infer_frame(dev(pts))
    return {k: eng.fetch(0, k).clone() for k in ("rpn", "cls", "box", "dir")}


@pytest.mark.parametrize("name", list(FRAMES) + ["lidar"])
def test_switch_on_equals_switch_off(eng, clouds, name):
    eng.set_sparse_conv1(True)
    eng.set_tile_skip(True)
    on = tensors(eng, clouds[name])
    assert eng.tile_skip_active()
    eng.set_tile_skip(False)
    off = tensors(eng, clouds[name])
    assert not eng.tile_skip_active()
    with pytest.raises(RuntimeError):
        eng.fetch(0, "tile_flags")  # a pass with the switch off builds none
    eng.set_tile_skip(True)
    d = {k: float((on[k] - off[k]).abs().max()) for k in on}
    line = (f"[tile skip] on vs off, {name}: max abs difference " + str({k: f"{v:.2e}" for k, v in d.items()})
            + f", exactly 0: {max(d.values()) == 0.0}")
    print(line)
    report(line)
    for k in on:
        assert bool(torch.isfinite(on[k]).all())
    assert max(d.values()) <= 1e-4, d


def test_frame_does_not_depend_on_its_batch(eng, clouds):
    """The same cloud at positions 0, 31, 32, 33 of a 34-frame pass (two stage groups) between empty and full clouds, and alone."""
    eng.set_sparse_conv1(True)
    eng.set_tile_skip(True)
    mine, empty, full = dev(clouds["lidar"]), dev(clouds["none"]), dev(clouds["full"])
    det1, cnt1 = eng.infer_frame(mine)
    cnt1 = cnt1.cpu().numpy().copy()
    det1 = det1.cpu().numpy().copy()
    flags1 = eng.fetch(0, "tile_flags").cpu().numpy().copy()
    assert cnt1[0] > 0 and eng.tile_skip_active()
    at = (0, 31, 32, 33)
    batch = [mine if f in at else (empty if f % 2 else full) for f in range(MAXB)]
    det_b, cnt_b = eng.infer_batch(batch)
    det_b, cnt_b = det_b.cpu().numpy(), cnt_b.cpu().numpy()
    assert eng.tile_skip_active()
    worst = 0.0
    for f in at:
        assert np.array_equal(eng.fetch(f, "tile_flags").cpu().numpy(), flags1)
        assert np.array_equal(cnt_b[f], cnt1)
        worst = max(worst, float(np.abs(det_b[f, :cnt1[0]] - det1[:cnt1[0]]).max()))
    print(f"[tile skip] frame alone vs positions {at} of {MAXB}: max row difference {worst:.2e}")
    assert worst <= 1e-5
    assert eng.fetch(1, "tile_flags").cpu().numpy().all() and not eng.fetch(2, "tile_flags").cpu().numpy().any()


def test_strip_fallback_is_inactive_and_unchanged(synth):
    """Maps 36 x 44 are no whole number of 16 x 16 tiles: the layers run main + strip launches and the path stays out of them."""
    over = dict(detection_range=[0.0, -8.8, -2.5, 14.4, 8.8, 8.5], max_voxels=16000)
    e = forced_engine(synth, make_cfg(synth, **over), 2)
    assert (e.H, e.W) == (36, 44)
    pts = synth.lidar_cloud("eight_20cm", seed=5)
    e.set_sparse_conv1(True)
    e.set_tile_skip(True)
    on = tensors(e, pts)
    assert not e.tile_skip_active()
    with pytest.raises(RuntimeError):
        e.fetch(0, "tile_flags")
    e.set_tile_skip(False)
    off = tensors(e, pts)
    assert not e.tile_skip_active()
    d = {k: float((on[k] - off[k]).abs().max()) for k in on}
    print("[tile skip] strip fallback, on vs off: " + str({k: f"{v:.2e}" for k, v in d.items()}))
    assert max(d.values()) <= 1e-4, d
