"""Sparse first convolution (-m gpu): the fused fp32 path lists the output pixels that see a pillar, runs a gather-GEMM over the
list and scatters into the zero-filled dense map.  Checked on the 72 x 88-cell grid of test_fused_frame_odd_level2_maps (maps
36 x 44, 1584 output pixels): the list against numpy, switch on against switch off (1e-4: the bar check_golden_samples sets for this
network under another summation order), the CPU oracle, independence of a frame from its batch, the empty frame."""
import numpy as np
import pytest
import torch

from conftest import load_pkg
from frame_check import compare_frame, gpu_logits, oracle_frame, report

pytestmark = pytest.mark.gpu

OVER = dict(detection_range=[0.0, -8.8, -2.5, 14.4, 8.8, 8.5])
GX, GY, H, W = 72, 88, 36, 44
MAXB = 34  # crosses PP_GROUP = 32


def make_cfg(synth, **over):
    cfg = synth.load_config("eight_20cm")
    cfg.update(OVER)
    cfg.update(over)
    cfg["device"] = torch.device("cuda:0")
    return cfg


def cloud_of_cells(cells):
    """One point in the centre of every (cx, cy) cell."""
    c = np.asarray(cells, np.float32).reshape(-1, 2)
    pts = np.zeros((c.shape[0], 4), np.float32)
    pts[:, 0] = (c[:, 0] + 0.5) * 0.2
    pts[:, 1] = -8.8 + (c[:, 1] + 0.5) * 0.2
    pts[:, 2] = 0.5
    pts[:, 3] = 0.3
    return pts


def even_cells(n):
    """n pillars in distinct even-even cells: each is seen by exactly one output pixel."""
    return [(2 * (i % H), 2 * ((7 * i) % W)) for i in range(n)]


BORDER = [(x, y) for x in range(GX) for y in range(GY) if x in (0, GX - 1) or y in (0, GY - 1)]
CRAFTED = {
    "none": (np.array([[-5.0, 0.0, 0.0, 0.1]], np.float32), 0),  # the only point lies outside the range
    "one": (cloud_of_cells(even_cells(1)), 1),
    "n15": (cloud_of_cells(even_cells(15)), 15),
    "n16": (cloud_of_cells(even_cells(16)), 16),
    "n17": (cloud_of_cells(even_cells(17)), 17),
    "full": (cloud_of_cells([(x, y) for x in range(GX) for y in range(GY)]), H * W),
    "corners": (cloud_of_cells([(0, 0), (GX - 1, 0), (0, GY - 1), (GX - 1, GY - 1)]), 4),
    "borders": (cloud_of_cells(BORDER), 2 * H + 2 * W - 4),
}


@pytest.fixture(scope="module")
def eng(synth):
    e = load_pkg("engine").Engine(make_cfg(synth), max_batch=MAXB)
    e.load_state_dict(synth.seeded_state_dict(6, cls_bias=-3.0))
    assert (e.H, e.W) == (H, W) and e.max_voxels >= GX * GY
    return e


@pytest.fixture(scope="module")
def lidar(synth):
    return synth.lidar_cloud("eight_20cm", seed=5)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def active_list(eng, frame):
    raw = eng.fetch(frame, "active").cpu().numpy()
    return int(raw[0]), raw[1:1 + int(raw[0])].copy()


def numpy_active(eng, frame):
    """Active output pixels from the frame's own pillar coordinates: 3x3 window, stride 2, padding 1."""
    n = int(eng.fetch(frame, "num").cpu().numpy()[0])
    coors = eng.fetch(frame, "coors").cpu().numpy()[:n]
    occ = np.zeros((GX + 2, GY + 2), bool)
    occ[coors[:, 0] + 1, coors[:, 1] + 1] = True
    act = np.zeros((H, W), bool)
    for ky in range(3):
        for kx in range(3):
            act |= occ[ky:ky + 2 * H:2, kx:kx + 2 * W:2]
    return n, np.flatnonzero(act.reshape(-1)).astype(np.int32)


@pytest.mark.parametrize("name", list(CRAFTED) + ["lidar"])
def test_active_list_against_numpy(eng, lidar, name):
    pts, want = CRAFTED[name] if name != "lidar" else (lidar, None)
    eng.set_sparse_conv1(True)
    eng.infer_frame(dev(pts))
    torch.cuda.synchronize()
    count, idx = active_list(eng, 0)
    pillars, ref = numpy_active(eng, 0)
    print(f"[sparse conv1] {name}: {pillars} pillars, {count} active pixels of {H * W}")
    assert count == ref.size
    assert np.array_equal(idx, ref)
    assert np.all(np.diff(idx) > 0)
    if want is not None:
        assert count == want
    else:
        assert pillars > 300


def tensors(eng, pts):
    eng.infer_frame(dev(pts))
    return {k: eng.fetch(0, k).clone() for k in ("rpn", "cls", "box", "dir")}


@pytest.mark.parametrize("name", list(CRAFTED) + ["lidar"])
def test_switch_on_equals_switch_off(eng, lidar, name):
    pts = CRAFTED[name][0] if name != "lidar" else lidar
    eng.set_sparse_conv1(True)
    on = tensors(eng, pts)
    active_list(eng, 0)  # the pass built a list
    eng.set_sparse_conv1(False)
    off = tensors(eng, pts)
    with pytest.raises(RuntimeError):
        eng.fetch(0, "active")  # the dense first conv builds none
    eng.set_sparse_conv1(True)
    d = {k: float((on[k] - off[k]).abs().max()) for k in on}
    line = f"[sparse conv1] on vs off, {name}: max abs difference " + str({k: f"{v:.2e}" for k, v in d.items()})
    print(line)
    report(line)
    for k in on:
        assert bool(torch.isfinite(on[k]).all())
    assert max(d.values()) <= 1e-4, d


@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_against_oracle(synth, lidar, norm):
    sd = synth.seeded_state_dict(6, norm=norm, cls_bias=-3.0)
    e = load_pkg("engine").Engine(make_cfg(synth), norm=norm)
    e.load_state_dict(sd)
    e.set_sparse_conv1(True)
    det, cnt = e.infer_frame(dev(lidar))
    cnt = cnt.cpu().numpy()
    assert active_list(e, 0)[0] > 300
    r = oracle_frame(synth, "eight_20cm", lidar, sd, norm, over=OVER)
    assert r["coors"].shape[0] > 300
    compare_frame(r, gpu_logits(e, 0), det[:cnt[0]].cpu().numpy(), cnt, 0, f"sparse conv1 72x88 grid, {norm} norm")


def test_frame_does_not_depend_on_its_batch(eng, lidar):
    """The same cloud at positions 0, 31, 32, 33 of a 34-frame pass (two stage groups) between empty and full clouds, and alone."""
    eng.set_sparse_conv1(True)
    mine, empty, full = dev(lidar), dev(CRAFTED["none"][0]), dev(CRAFTED["full"][0])
    det1, cnt1 = eng.infer_frame(mine)
    cnt1 = cnt1.cpu().numpy().copy()
    det1 = det1.cpu().numpy().copy()
    list1 = active_list(eng, 0)
    assert cnt1[0] > 0
    at = (0, 31, 32, 33)
    clouds = [mine if f in at else (empty if f % 2 else full) for f in range(MAXB)]
    det_b, cnt_b = eng.infer_batch(clouds)
    det_b, cnt_b = det_b.cpu().numpy(), cnt_b.cpu().numpy()
    worst = 0.0
    for f in at:
        c, idx = active_list(eng, f)
        assert c == list1[0] and np.array_equal(idx, list1[1])
        assert np.array_equal(cnt_b[f], cnt1)
        worst = max(worst, float(np.abs(det_b[f, :cnt1[0]] - det1[:cnt1[0]]).max()))
    print(f"[sparse conv1] frame alone vs positions {at} of {MAXB}: max row difference {worst:.2e}")
    assert worst <= 1e-5
    assert active_list(eng, 1)[0] == 0 and active_list(eng, 2)[0] == H * W


def test_empty_frame(eng):
    """No point in range: the list is empty, every plane is exactly zero, and the statistics of an all-zero plane give
    scale 1 / sqrt(eps) and shift 0 -- relu(norm(0)) = 0 throughout, nothing is NaN, nothing is detected."""
    eng.set_sparse_conv1(True)
    det, cnt = eng.infer_frame(dev(CRAFTED["none"][0]))
    torch.cuda.synchronize()
    assert int(cnt[0]) == 0
    assert active_list(eng, 0)[0] == 0
    rpn = eng.fetch(0, "rpn")
    assert bool(torch.isfinite(rpn).all()) and float(rpn.abs().max()) == 0.0
    for k in ("cls", "box", "dir"):
        assert bool(torch.isfinite(eng.fetch(0, k)).all())
