"""GPU parity tests (-m gpu): the HIP path, called through the C ABI (libpp_hip.so via the drop-in
classes), against the oracle and the golden vectors captured from the reference.
Integer / index stages: bit-exact.  Float stages: tolerance written at each assert
(north star: boxes and scores within 1e-3 fp32)."""
import hashlib

import numpy as np
import pytest
import torch

from conftest import ROOT, golden, load_pkg
from oracle import c_oracle as C
from oracle import pp_oracle as O

pytestmark = pytest.mark.gpu

CONFIGS = ("eight_20cm", "ntusl_10cm", "nuscene")


def sha(*arrs):
    h = hashlib.sha256()
    for a in arrs:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def make_cfg(synth, name, **over):
    cfg = synth.load_config(name)
    cfg.update(over)
    cfg["device"] = torch.device("cuda:0")
    return cfg


@pytest.fixture(scope="module")
def fw():
    pkg = load_pkg()
    pkg.install()
    import framework.voxel_generator as vg
    import framework.anchor_assigner as aa
    import framework.dataset as ds
    import framework.inference as inf
    import framework.nms as nms
    import framework.box_torch_ops as bto
    import networks.pointpillars8_shared as shared
    import networks.pointpillars8_export as export
    return dict(vg=vg, aa=aa, ds=ds, inf=inf, nms=nms, bto=bto, shared=shared, export=export)


def test_native_library_is_loaded():
    lib = load_pkg("_lib")
    assert lib.load().pp_version() >= 1
    with open("/proc/self/maps") as f:
        assert "libpp_hip.so" in f.read()


# ------------------------------------------------------------------ a2 voxeliser (bit-exact)
@pytest.mark.parametrize("name", CONFIGS)
def test_voxelize_small_break(name, fw, synth):
    g = golden(f"voxel_small_{name}")
    cfg = make_cfg(synth, name, max_voxels=int(g["max_voxels"]), max_num_points=int(g["max_num_points"]))
    v, c, n = fw["vg"].VoxelGenerator(cfg).generate(g["points"])
    assert v.shape[0] == 900
    assert np.array_equal(c, g["coors"]) and np.array_equal(n, g["num"]) and np.array_equal(v, g["voxels"])


@pytest.mark.parametrize("name", CONFIGS)
def test_voxelize_full(name, fw, synth):
    g = golden(f"voxel_full_{name}")
    cfg = make_cfg(synth, name)
    pts = synth.lidar_cloud(name, seed=1000)
    v, c, n = fw["vg"].VoxelGenerator(cfg).generate(pts)
    assert np.array_equal(c, g["coors"]) and np.array_equal(n, g["num"])
    assert sha(v) == str(g["voxels_sha"])


def test_voxelize_edges_and_empty(fw, synth):
    g = golden("voxel_edge")
    cfg = make_cfg(synth, "eight_20cm")
    vgen = fw["vg"].VoxelGenerator(cfg)
    v, c, n = vgen.generate(g["points"])
    assert np.array_equal(c, g["coors"]) and np.array_equal(n, g["num"]) and np.array_equal(v, g["voxels"])
    v, c, n = vgen.generate(np.zeros((0, 4), np.float32))
    assert v.shape == (0, 15, 4) and c.shape == (0, 3) and n.shape == (0,)
    out = np.full((50, 4), 1e6, np.float32)  # every point outside the range
    v, c, n = vgen.generate(out)
    assert v.shape[0] == 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_voxelize_random_vs_oracle(seed, fw, synth):
    """Dense + duplicate-heavy clouds (many points per cell, pathological single cell) against the C oracle."""
    rng = np.random.default_rng(seed)
    cfg = make_cfg(synth, "eight_20cm", max_voxels=500 * seed, max_num_points=7)
    s = O.voxel_setup(synth.load_config("eight_20cm"))
    pts = np.concatenate([rng.uniform(-12, 12, (30000, 4)), np.tile([[3.05, 4.05, 0.0, 0.5]], (5000, 1)),
                          rng.uniform(-100, 100, (5000, 4))]).astype(np.float32)
    rng.shuffle(pts)
    v, c, n = fw["vg"].VoxelGenerator(cfg).generate(pts)
    vo, co, no = C.points_to_voxels(pts, s["voxel_size"], s["offset"], s["grid_size"], cfg["max_voxels"], 7)
    assert np.array_equal(c, co) and np.array_equal(n, no) and np.array_equal(v, vo)


def test_voxelize_idempotent_on_own_output(fw, synth):
    """Size-independent property at full size: re-voxelising the concatenated pillar contents in
    pillar order reproduces the same pillars."""
    cfg = make_cfg(synth, "eight_20cm")
    vgen = fw["vg"].VoxelGenerator(cfg)
    v, c, n = vgen.generate(synth.lidar_cloud("eight_20cm", seed=5))
    flat = np.concatenate([v[i, :n[i]] for i in range(v.shape[0])])
    v2, c2, n2 = vgen.generate(flat)
    assert np.array_equal(c, c2) and np.array_equal(n, n2) and np.array_equal(v, v2)


# ------------------------------------------------------------------ a3/a4 anchors + mask (bit-exact)
def test_anchor_mask_full(fw, synth):
    g = golden("anchors_eight_20cm")
    cfg = make_cfg(synth, "eight_20cm")
    fw["vg"].VoxelGenerator(cfg)
    aa = fw["aa"].AnchorAssigner(cfg)
    assert sha(aa.anchors) == str(g["anchors_sha"]) and sha(aa.anchors_coors) == str(g["coors_sha"])
    coors = golden("voxel_full_eight_20cm")["coors"]
    m = aa.create_mask(coors, cfg["grid_size"], None, None)
    assert m.dtype == np.bool_ and int(m.sum()) == int(g["mask_count"])
    assert np.array_equal(np.packbits(m), g["mask_bits"])
    assert not aa.create_mask(np.zeros((0, 3), np.int32)).any()  # empty frame -> nothing kept


@pytest.mark.parametrize("name", ["ntusl_10cm", "nuscene"])
def test_anchor_mask_other_grids(name, fw, synth):
    cfg = make_cfg(synth, name)
    vgen = fw["vg"].VoxelGenerator(cfg)
    aa = fw["aa"].AnchorAssigner(cfg)
    v, c, n = vgen.generate(synth.lidar_cloud(name, seed=1000))
    s = O.voxel_setup(synth.load_config(name))
    a = O.make_anchors(s)
    assert np.array_equal(aa.anchors, a["anchors"]) and np.array_equal(aa.anchors_coors, a["anchors_coors"])
    assert np.array_equal(aa.create_mask(c), C.create_mask(c, s["grid_size"], a["anchors_coors"]))


# ------------------------------------------------------------------ a6/a7 PFN + scatter
def test_pfn(fw, synth):
    g = golden("pfn_eight_20cm")
    cfg = make_cfg(synth, "eight_20cm")
    fw["vg"].VoxelGenerator(cfg)
    net = fw["shared"].PointPillars(cfg)
    net.load_state_dict(synth.seeded_state_dict(0))
    d = torch.device("cuda:0")
    out = net.pillar_point_net(torch.from_numpy(g["voxels"]).to(d), torch.from_numpy(g["num"]).to(d),
                               torch.from_numpy(g["coors"]).to(d)).cpu().numpy()
    np.testing.assert_allclose(out, g["out"], rtol=0, atol=2e-5)  # fp32 PFN, tolerance 2e-5 abs


def test_pfn_T100_and_scatter(fw, synth):
    """nuscene: T=100 exercises the multi-chunk point loop; scatter against the oracle (exact copy)."""
    cfg = make_cfg(synth, "nuscene")
    vgen = fw["vg"].VoxelGenerator(cfg)
    net = fw["shared"].PointPillars(cfg)
    sd = synth.seeded_state_dict(0)
    net.load_state_dict(sd)
    v, c, n = vgen.generate(synth.lidar_cloud("nuscene", seed=3))
    s = O.voxel_setup(synth.load_config("nuscene"))
    d = torch.device("cuda:0")
    feat = net.pillar_point_net(torch.from_numpy(v).to(d), torch.from_numpy(n).to(d), torch.from_numpy(c).to(d))
    ref = O.pfn(v, n, c, sd, s)
    np.testing.assert_allclose(feat.cpu().numpy(), ref, rtol=0, atol=5e-5)
    canvas = net.middle_feature_extractor(feat, torch.from_numpy(c).to(d)).cpu().numpy()
    assert np.array_equal(canvas, O.scatter(feat.cpu().numpy(), c, s["grid_size"]))


def test_bad_stage_inputs_do_not_reach_the_device(fw, synth):
    """Out-of-grid coordinates and an over-long point count are skipped / clamped by the kernels; wrong tensors raise."""
    cfg = make_cfg(synth, "nuscene")
    vgen = fw["vg"].VoxelGenerator(cfg)
    net = fw["shared"].PointPillars(cfg)
    d = torch.device("cuda:0")
    v, c, n = vgen.generate(synth.lidar_cloud("nuscene", seed=3, n_points=4000))
    vt, ct, nt = torch.from_numpy(v).to(d), torch.from_numpy(c).to(d), torch.from_numpy(n).to(d)
    feat = net.pillar_point_net(vt, nt, ct)
    good = net.middle_feature_extractor(feat, ct)
    bad_c = ct.clone()
    bad_c[0, 0] = 100000   # far outside the 512 x 480 grid
    bad_c[1, 1] = -7
    canvas = net.middle_feature_extractor(feat, bad_c)
    torch.cuda.synchronize()
    ref = good.clone()
    for k in (0, 1):       # the two bad pillars are simply absent
        ref[0, :, int(c[k, 0]), int(c[k, 1])] = 0
    assert torch.equal(canvas, ref)
    nt2 = nt.clone()
    nt2[0] = 10 ** 6       # a count beyond T reads at most the pillar's own T slots
    f2 = net.pillar_point_net(vt, nt2, ct)
    torch.cuda.synchronize()
    assert torch.isfinite(f2).all() and torch.equal(f2[1:], feat[1:])
    with pytest.raises(TypeError):
        net.middle_feature_extractor(feat, ct.long())
    with pytest.raises(TypeError):
        net.middle_feature_extractor(feat.cpu(), ct)
    with pytest.raises(ValueError):
        net.pillar_point_net(vt[:, :7], nt, ct)


# ------------------------------------------------------------------ a8/a9 backbone + head (small grids, golden)
def small_cfg(synth, gx, gy):
    cfg = synth.load_config("eight_20cm")
    cfg["detection_range"] = [0.0, 0.0, -2.5, 0.2 * gx, 0.2 * gy, 8.5]
    cfg["max_voxels"] = 2000
    cfg["device"] = torch.device("cuda:0")
    return cfg


@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_backbone_small(norm, fw, synth):
    g = golden(f"backbone_small_{norm}")
    cfg = small_cfg(synth, 64, 48)
    fw["vg"].VoxelGenerator(cfg)
    net = (fw["shared"] if norm == "instance" else fw["export"]).PointPillars(cfg)
    net.load_state_dict(synth.seeded_state_dict(0, norm=norm))
    y = net.rpn(torch.from_numpy(g["x"]).cuda()).cpu().numpy()
    assert y.shape == g["y"].shape
    # fp32 MFMA (k-ordered fma chain) vs torch CPU conv: 16 stacked convs + norms, tolerance 2e-4 abs on O(1) activations
    np.testing.assert_allclose(y, g["y"], rtol=0, atol=2e-4)


@pytest.mark.parametrize("force", ["g1x1", "wino tw8", "wino tw4", "wino tw8 w1x4 bx1 kc4", "wino tw8 w2x4", "wino4 tw4 bx2", "wino4 tw8 bx1", "wino4 tw8 bx2", "wino6 tw4",
                                   "k3s1 tw16 w1x4 t4x4", "k3s1 tw4 w2x2 t2x2", "k3s1 tw8 w2x2 t4x5"])
def test_backbone_forced_tiling(force, fw, synth, monkeypatch):
    """Every tiling family (Winograd F(2x2,3x3) and direct, exact and masked-edge shapes) must give the
    same network output, whatever the autotuner would pick."""
    monkeypatch.setenv("PP_FORCE_VARIANT", force)
    g = golden("backbone_small_instance")
    cfg = small_cfg(synth, 64, 48)
    fw["vg"].VoxelGenerator(cfg)
    net = fw["shared"].PointPillars(cfg)
    net.load_state_dict(synth.seeded_state_dict(0))
    y = net.rpn(torch.from_numpy(g["x"]).cuda()).cpu().numpy()
    np.testing.assert_allclose(y, g["y"], rtol=0, atol=2e-4)
    if force == "g1x1":  # the head has a persistent 1x1 variant too: oracle head on the same features
        sd = synth.seeded_state_dict(0)
        p = net.heads(torch.from_numpy(g["y"]).cuda())
        cls, box, dr = O.head(g["y"], sd)
        np.testing.assert_allclose(p["cls_preds"].cpu().numpy(), cls, rtol=0, atol=5e-5)
        np.testing.assert_allclose(p["box_preds"].cpu().numpy(), box, rtol=0, atol=5e-5)
        np.testing.assert_allclose(p["dir_preds"].cpu().numpy(), dr, rtol=0, atol=5e-5)


C16_SHAPES = ["w2x2 t1x5 40x8 o2", "w2x2 t1x5 80x4 o2", "w2x2 t1x5 20x16 o2", "w4x1 t1x5 20x8 o2", "w4x1 t1x5 40x4 o2",
              "w1x4 t2x5 80x8 o1", "w2x2 t2x5 40x8 o1", "w2x2 t2x5 20x16 o1", "w2x2 t1x5 40x8 o1", "w4x1 t1x5 20x8 o1",
              "w4x2 t1x5 40x8 o2", "w4x2 t1x5 20x16 o2", "w2x4 t1x5 80x8 o2"]  # the last three: eight-wave workgroups


@pytest.mark.parametrize("force,mode,tol", [(f, "bf16x3", 5e-4) for f in C16_SHAPES] + [("w2x2 t1x5 40x8 o2", "fp16", 0.03), ("w1x4 t2x5 80x8 o1", "bf16", 0.2)])
def test_backbone_conv16_forced_tiling(force, mode, tol, fw, synth, monkeypatch):
    """Every tile shape of the 16-bit operand convolution kernels (conv16.hip: one / two workgroups per CU, 64 / 128 rows, 20- to
    80-pixel-wide tiles, stride 1 and 2) pinned on the golden small grid (maps 32 x 24 and 16 x 12: every tile overhangs the map,
    so the masked edges and the zero padding are what is tested; the 8 x 6 level keeps its fp32 tilings -- width 6), whatever the
    tuner would pick.  bf16x3 at a bar that only a correct kernel meets (observed 1.0e-4 on every shape); one shape each in fp16 / bf16."""
    monkeypatch.setenv("PP_FORCE_VARIANT", force)
    g = golden("backbone_small_instance")
    cfg = small_cfg(synth, 64, 48)
    fw["vg"].VoxelGenerator(cfg)
    net = fw["shared"].PointPillars(cfg)
    net.load_state_dict(synth.seeded_state_dict(0))
    net.precision(mode)
    til = net._eng.layer_tilings()
    forced = [t["tiling"] for t in til if t["kind"] == 0 and force in t["tiling"]]
    assert forced, [t["tiling"] for t in til]  # the shape really runs on at least one layer (rows must be a multiple of its 64 / 128)
    y = net.rpn(torch.from_numpy(g["x"]).cuda()).cpu().numpy()
    dev = float(np.abs(y - g["y"]).max())
    print(f"[conv16 forced] {force} {mode}: {len(forced)} layers, max deviation from the reference's backbone output {dev:.2e}")
    assert dev <= tol, (force, mode, dev)
    net.precision("fp32")


@pytest.mark.parametrize("force,strips", [("wino4 tw4 bx2", "2"), ("wino4 tw8 bx1", "2"), ("wino4 tw8 bx2", "2"), ("wino4 tw4 bx2", "0"),
                                          ("wino6 tw4", "2"), ("wino6 tw4", "0")])
def test_backbone_wino4_edge_maps(force, strips, fw, synth, monkeypatch):
    """wino4_mfma (and wino6_mfma: its 36 x 44 level -- the other two are no multiples of 4 and keep other kernels -- as 2 x 2 main tiles +
    4 x 64 / 64 x 4 strip tiles, or as 3 x 3 rounded-up tiles with masked lanes) on maps that are no multiple of its tile: 72 x 88 canvas -> 36 x 44 (dwordx4 rows), 18 x 22 (width = 2 mod 4:
    the dwordx2 form of the epilogue) and 9 x 11 (odd: another kernel takes over) maps, with the region launches forced
    (PP_W4_STRIPS=2: whole main tiles + right / bottom strips of thin tiles, regions starting off a multiple of 4) and disabled,
    against the CPU oracle's backbone."""
    monkeypatch.setenv("PP_FORCE_VARIANT", force)
    monkeypatch.setenv("PP_W4_STRIPS", strips)
    cfg = small_cfg(synth, 72, 88)
    fw["vg"].VoxelGenerator(cfg)
    net = fw["shared"].PointPillars(cfg)
    sd = synth.seeded_state_dict(4)
    net.load_state_dict(sd)
    x = np.random.default_rng(11).standard_normal((1, 64, 72, 88)).astype(np.float32)
    x[:, :, ::3, ::2] = 0.0
    y = net.rpn(torch.from_numpy(x).cuda()).cpu().numpy()
    ref = O.backbone(x, sd)
    assert y.shape == ref.shape
    np.testing.assert_allclose(y, ref, rtol=0, atol=2e-4)


_RCCL_CHILD = r"""
import importlib, os, sys
import torch
import torch.distributed as dist
sys.path.insert(0, sys.argv[1])
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
os.environ["MASTER_ADDR"] = "127.0.0.1"
os.environ["MASTER_PORT"] = sys.argv[2]
# the real RCCL backend, initialised before any other GPU work of this process
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
shard = importlib.import_module("3d_object_detection_amd.shard")
dev = torch.device("cuda", 0)
rows, ncnt, pad = 900, 13, 4
g = shard.DetectionGatherer(rows, ncnt, pad, dev, force_collective=True)
assert g.collective
side = torch.cuda.Stream()
ok = True
with torch.cuda.stream(side):                      # a non-default stream, as bench.py's compute stream
    for step in range(3):
        f = 3 if step < 2 else 0                   # the last step: a rank without frames still takes part
        det = torch.randn((f, rows, 9), device=dev) * (step + 1)
        cnt = torch.randint(0, 900, (f, ncnt), dtype=torch.int32, device=dev)
        out = g.gather(det, cnt)                   # enqueue only
        d, c = g.unpack([f], out)                  # host-known count
        side.synchronize()
        ok &= torch.equal(d[0], det) and torch.equal(c[0], cnt) and (f == 0 or d[0].data_ptr() != det.data_ptr())
        if not ok: print('step', step, 'mismatch'); break
d2, c2 = shard.gather_detections(torch.ones((2, rows, 9), device=dev), torch.full((2, ncnt), 7, dtype=torch.int32, device=dev), force_collective=True)
torch.cuda.synchronize()
ok &= d2[0].shape == (2, rows, 9) and bool((d2[0] == 1).all()) and bool((c2[0] == 7).all())
t = torch.tensor([1.5], dtype=torch.float64, device=dev)
dist.all_reduce(t, op=dist.ReduceOp.MAX)           # the max-over-ranks timing of bench.py
ok &= float(t.item()) == 1.5
dist.barrier()
dist.destroy_process_group()
print("RCCL_OK" if ok else "RCCL_MISMATCH")
"""


def test_rccl_single_rank_gather():
    """The multi-GPU leg's collective on the real backend: a child process initialises `nccl` (= RCCL) with world_size 1 BEFORE any
    other GPU work and drives bench.py's per-step exchange on device tensors -- pack into the preallocated block, all_gather, trim
    from host-known counts, on a side stream, three steps incl. an empty shard -- plus the one-shot form and the max-over-ranks
    all_reduce.  (RCCL refuses two ranks on one device, so world_size 1 is what a one-GPU box can run; the N = 2/4/8 runs are the
    driver's.  SURVEY 8(e); no reference counterpart.)"""
    import socket
    import subprocess
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    r = subprocess.run([sys.executable, "-c", _RCCL_CHILD, ROOT, str(port)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RCCL_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_backbone_wino6_all_levels(fw, synth, monkeypatch):
    """wino6_mfma -- Winograd F(4x4,3x3), positions split over the waves, all vector-memory operations counted by the kernel itself
    (csrc/wino6.hip) -- forced on every stride-1 3x3 convolution: 128 x 128 canvas -> maps 64, 32 and 16 (whole
    16 x 16-pixel tiles at all three levels, 16 / 4 / 1 tiles per frame: more workgroups than items at the coarse levels), against
    the CPU oracle's backbone (networks/pointpillars8_shared.py:114-181)."""
    monkeypatch.setenv("PP_FORCE_VARIANT", "wino6")
    cfg = small_cfg(synth, 128, 128)
    fw["vg"].VoxelGenerator(cfg)
    net = fw["shared"].PointPillars(cfg)
    sd = synth.seeded_state_dict(4)
    net.load_state_dict(sd)
    til = [t["tiling"] for t in net._eng.layer_tilings() if t["kind"] == 0 and t["stride"] == 1]
    assert len(til) == 13 and all("wino6" in t for t in til), til
    x = np.random.default_rng(12).standard_normal((1, 64, 128, 128)).astype(np.float32)
    x[:, :, ::3, ::2] = 0.0
    y = net.rpn(torch.from_numpy(x).cuda()).cpu().numpy()
    ref = O.backbone(x, sd)
    dev = float(np.abs(y - ref).max())
    print(f"[wino6] 13 layers on F(4x4,3x3): max deviation from the oracle's backbone output {dev:.2e}")
    np.testing.assert_allclose(y, ref, rtol=0, atol=2e-4)


def test_head_layout(fw, synth):
    g = golden("head_small")
    cfg = small_cfg(synth, 16, 12)
    fw["vg"].VoxelGenerator(cfg)
    net = fw["shared"].PointPillars(cfg)
    net.load_state_dict(synth.seeded_state_dict(0))
    p = net.heads(torch.from_numpy(g["x"]).cuda())
    np.testing.assert_allclose(p["cls_preds"].cpu().numpy(), g["cls"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(p["box_preds"].cpu().numpy(), g["box"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(p["dir_preds"].cpu().numpy(), g["dir"], rtol=0, atol=2e-5)


# ------------------------------------------------------------------ a11/a12 box math
def test_box_math(fw):
    g = golden("boxmath")
    b = fw["bto"]
    dec = b.box_decode(torch.from_numpy(g["enc"]).cuda(), torch.from_numpy(g["anchors"]).cuda()).cpu().numpy()
    np.testing.assert_allclose(dec, g["dec_np"], rtol=1e-6, atol=1e-6)
    cor = b.center_to_corner_box2d(torch.from_numpy(g["dec_np"][:, :2].copy()).cuda(), torch.from_numpy(g["dec_np"][:, 3:5].copy()).cuda(),
                                   torch.from_numpy(g["dec_np"][:, 6].copy()).cuda()).cpu().numpy()
    np.testing.assert_allclose(cor, g["cor_np"], rtol=0, atol=1e-5)
    st = b.corner_to_standup_nd(torch.from_numpy(g["cor_np"]).cuda()).cpu().numpy()
    assert np.array_equal(st, g["st_np"])


# ------------------------------------------------------------------ a13/a14 NMS
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300, 1000])
def test_nms_aabb(n, fw):
    g = golden("nms_aabb")
    assert fw["nms"].nms_gpu(g[f"dets_{n}"], 0.1) == [int(v) for v in g[f"keep_{n}"]]


def test_nms_empty_and_ties(fw):
    assert fw["nms"].nms_gpu(np.zeros((0, 5), np.float32), 0.1) == []
    d = np.array([[0, 0, 4, 4, 0.5], [10, 10, 14, 14, 0.5], [0.5, 0.5, 4.5, 4.5, 0.5]], np.float32)
    assert fw["nms"].nms_gpu(d, 0.1) == O.nms_aabb(d, 0.1) == [0, 1]  # equal scores: lower index first


def test_nms_aabb_large_vs_oracle(fw):
    rng = np.random.default_rng(11)
    n = 4096
    ctr = rng.uniform(-60, 60, (n, 2))
    wh = rng.uniform(0.5, 6.0, (n, 2))
    d = np.concatenate([ctr - wh / 2, ctr + wh / 2, rng.permutation(n)[:, None] / n], axis=1).astype(np.float32)
    assert fw["nms"].nms_gpu(d, 0.1) == C.nms_aabb(d, 0.1)


def _exact_iou(b1, b2):
    """fp64 IoU of two rotated boxes (cx,cy,dx,dy,angle) by Sutherland-Hodgman clipping: an arbiter that has no
    in/out tests on fp32 corner coordinates."""
    def corners(b):
        c, s = np.cos(float(b[4])), np.sin(float(b[4]))
        pts = np.array([[-0.5, -0.5], [-0.5, 0.5], [0.5, 0.5], [0.5, -0.5]]) * np.array([float(b[2]), float(b[3])])
        return pts @ np.array([[c, -s], [s, c]]) + np.array([float(b[0]), float(b[1])])  # eval/iou.py:351-374: x' = c x + s y, y' = -s x + c y

    def area(p):
        return 0.5 * abs(sum(p[i][0] * p[(i + 1) % len(p)][1] - p[(i + 1) % len(p)][0] * p[i][1] for i in range(len(p)))) if len(p) >= 3 else 0.0

    poly, clip = [tuple(x) for x in corners(b1)], corners(b2)
    if area(list(map(tuple, clip))) and np.cross(clip[1] - clip[0], clip[2] - clip[1]) < 0:
        clip = clip[::-1]
    for i in range(4):
        a_, b_ = clip[i], clip[(i + 1) % 4]
        e = b_ - a_
        out = []
        for j in range(len(poly)):
            p_, q_ = np.array(poly[j]), np.array(poly[(j + 1) % len(poly)])
            sp, sq = np.cross(e, p_ - a_), np.cross(e, q_ - a_)
            if sp >= 0:
                out.append(tuple(p_))
            if (sp >= 0) != (sq >= 0):
                t = sp / (sp - sq)
                out.append(tuple(p_ + t * (q_ - p_)))
        poly = out
        if not poly:
            break
    inter = area(poly)
    a1, a2 = float(b1[2]) * float(b1[3]), float(b2[2]) * float(b2[3])
    return inter / (a1 + a2 - inter)


def test_rotated_iou_and_nms(fw):
    g = golden("nms_rotated")
    m = fw["nms"].rotate_iou_gpu(g["boxes"], g["boxes"])
    ok = np.isfinite(g["iou"])
    dev = np.abs(m - g["iou"])
    out = np.argwhere(ok & ~(dev < 1e-4))
    # devRotateIoU decides "corner inside the other box" on fp32 coordinates: where a corner lies ON an edge (identical /
    # edge-sharing boxes) one ulp of sinf/cosf flips the test and a whole triangle of the intersection polygon.  Every pair
    # that leaves the 1e-4 band must therefore be such a pair -- shown by an fp64 clipping arbiter: the reference's own
    # value is at least as far from the true IoU as ours is from the reference -- and there may be only a handful.
    worst = 0.0
    for i, j in out:
        ex = _exact_iou(g["boxes"][i], g["boxes"][j])
        e_gpu, e_ref = abs(float(m[i, j]) - ex), abs(float(g["iou"][i, j]) - ex)
        worst = max(worst, e_gpu)
        assert e_gpu <= 1e-4 or e_ref > 1e-4, (i, j, float(m[i, j]), float(g["iou"][i, j]), ex)
    print(f"[rotated iou] {ok.sum()} finite pairs, max dev inside band {dev[ok & (dev < 1e-4)].max():.2e}, {len(out)} degenerate pairs "
          f"(GPU vs fp64 arbiter worst {worst:.2e})")
    assert len(out) <= 0.005 * ok.sum()
    assert fw["nms"].rotate_nms_gpu(g["dets"], 0.1) == [int(v) for v in g["keep"]]
    assert fw["nms"].rotate_nms_gpu(g["dets200"], 0.1) == [int(v) for v in g["keep200"]]


# ------------------------------------------------------------------ a10/a15 whole frame: tests/test_gpu_frames.py
def test_postprocess_stage_exact(fw, synth):
    """Post-processing fed with the ORACLE's head outputs: selection is integer work, so the kept
    anchors must match exactly and the boxes to 1e-5."""
    eng_mod = load_pkg("engine")
    cfg = make_cfg(synth, "nuscene")
    fw["vg"].VoxelGenerator(cfg)
    eng = eng_mod.Engine(cfg)
    rng = np.random.default_rng(5)
    A = eng.A
    # tie-free logits on a shuffled grid; ~3 % above the 0.05 threshold per class, > 1000 candidates
    logits = (rng.permutation(A).astype(np.float32) / A) * 8.0 - 10.6
    box = (rng.standard_normal((A, 7)) * 0.3).astype(np.float32)
    dr = rng.standard_normal((A, 2)).astype(np.float32)
    mask = rng.random(A) < 0.7
    s = O.voxel_setup(synth.load_config("nuscene"))
    a = O.make_anchors(s)
    for mode, name in ((0, "aabb"), (1, "rotated")):
        det, cnt = eng.postprocess(torch.from_numpy(logits).cuda(), torch.from_numpy(box).cuda(), torch.from_numpy(dr).cuda(),
                                   torch.from_numpy(mask).cuda(), nms_mode=mode)
        cnt = cnt.cpu().numpy()
        det = det[:cnt[0]].cpu().numpy()
        ref, counts = O.postprocess(logits, box, dr, mask, a["anchors"], a["class_masks"], cfg["center_limit"], name)
        assert list(cnt[1:4]) == counts, (mode, cnt, counts)
        np.testing.assert_allclose(det, ref, rtol=0, atol=2e-5)
    # no candidate at all
    det, cnt = eng.postprocess(torch.full((A,), -20.0).cuda(), torch.from_numpy(box).cuda(), torch.from_numpy(dr).cuda(),
                               torch.from_numpy(mask).cuda())
    assert int(cnt[0]) == 0


def test_batched_frames_equal_single_frames(fw, synth):
    """pp_infer_batch (frame = grid.z of the conv launches, per-frame InstanceNorm statistics) must give the
    same detections as separate pp_infer_frame calls, including ragged point counts and an empty cloud."""
    eng_mod = load_pkg("engine")
    cfg = make_cfg(synth, "nuscene")
    fw["vg"].VoxelGenerator(cfg)
    sd = synth.seeded_state_dict(2, cls_bias=-3.0)
    eng = eng_mod.Engine(cfg, max_batch=3)
    eng.load_state_dict(sd)
    clouds = [torch.from_numpy(synth.lidar_cloud("nuscene", seed=10)).cuda(),
              torch.from_numpy(synth.lidar_cloud("nuscene", seed=11, n_points=5000)).cuda(),
              torch.zeros((0, 4), dtype=torch.float32).cuda()]
    det_b, cnt_b = eng.infer_batch(clouds)
    for i, c in enumerate(clouds):
        d1, c1 = eng.infer_frame(c)
        assert np.array_equal(c1.cpu().numpy()[:4], cnt_b[i].cpu().numpy()[:4])
        k = int(c1[0])
        np.testing.assert_allclose(det_b[i, :k].cpu().numpy(), d1[:k].cpu().numpy(), rtol=0, atol=1e-5)
    assert int(cnt_b[2, 0]) == 0


def _assert_rows_close(a, b, rel=1e-5):
    """Detection rows [x y z w l h r score label] equal up to `rel` of the row's largest extent (the decode multiplies
    the logit noise by the anchor diagonal / exponentiates it), angles compared modulo 2 pi, labels exactly."""
    assert a.shape == b.shape
    if a.size == 0:
        return
    ext = np.maximum(1.0, np.abs(b[:, :6]).max(axis=1, keepdims=True))
    assert (np.abs(a[:, :6] - b[:, :6]) <= rel * ext).all(), float((np.abs(a[:, :6] - b[:, :6]) / ext).max())
    dr = np.abs(a[:, 6] - b[:, 6])
    dr = np.minimum(dr, np.abs(dr - 2 * np.pi))
    assert (dr <= rel).all(), float(dr.max())
    assert (np.abs(a[:, 7] - b[:, 7]) <= rel).all()
    assert np.array_equal(a[:, 8], b[:, 8])


def test_full_size_batch_properties(fw, synth):
    """BASELINE.json's metric workload (eight_20cm, 800x800 BEV) at a batch that spans TWO stage groups
    (PP_GROUP = 32 frames per integer-stage launch -> 34 frames = 32 + 2: the second iteration of the voxelise / mask / PFN and
    post-processing group loops of frame.hip runs), ragged clouds and empty frames on both sides of the boundary.
    Size-independent properties instead of the (too slow) oracle: frame independence (each frame of
    the batch equals its own pp_infer_frame; counts bit-exact, boxes to 1e-5 of the row's extent, logits to 1e-5), permutation
    equivariance and repeatability of the same call (all within 1e-5: the launch plan of a context -- tilings AND the
    Winograd main / strip split -- is fixed for its max_batch, not for the frames of a pass, so only the order of the fp64
    statistics atomics and the per-wave grouping of the 1x1 GEMMs' fp32 partial sums move)."""
    eng_mod = load_pkg("engine")
    cfg = make_cfg(synth, "eight_20cm")
    fw["vg"].VoxelGenerator(cfg)
    NB = 34
    eng = eng_mod.Engine(cfg, max_batch=NB)
    eng.load_state_dict(synth.seeded_state_dict(5, cls_bias=-3.0))
    sizes = [None, 90000, 30000, 7, 120000, 1] + [None] * 24 + [0, 50000, 12000, 0]   # frames 30 | 31 || 32 | 33 around the group boundary
    assert len(sizes) == NB
    clouds = []
    for i, n in enumerate(sizes):
        pts = synth.lidar_cloud("eight_20cm", seed=40 + i, n_points=n) if n != 0 else np.zeros((0, 4), np.float32)
        clouds.append(torch.from_numpy(pts).cuda())
    det_b, cnt_b = eng.infer_batch(clouds)
    det_b, cnt_b = det_b.cpu().numpy().copy(), cnt_b.cpu().numpy().copy()
    assert int(cnt_b[30, 0]) == 0 and int(cnt_b[33, 0]) == 0
    assert (cnt_b[:3, 0] > 0).all() and cnt_b[31, 0] > 0 and cnt_b[32, 0] > 0
    # frame independence, on both sides of the group boundary (round 2 needed 1e-4 here: launch_conv chose full tiles or
    # main + strip launches by the frames of the pass, which regrouped the InstanceNorm partial sums by ~3e-5)
    logits_b = {i: {k: eng.fetch(i, k).cpu().numpy() for k in ("cls", "box", "dir")} for i in (0, 32)}
    for i in (0, 3, 5, 30, 31, 32, 33):
        d1, c1 = eng.infer_frame(clouds[i])
        assert np.array_equal(c1.cpu().numpy()[:4], cnt_b[i][:4]), i
        k = int(c1[0])
        _assert_rows_close(det_b[i, :k], d1[:k].cpu().numpy())
        if i in logits_b:
            for name, t in logits_b[i].items():
                np.testing.assert_allclose(eng.fetch(0, name).cpu().numpy(), t, rtol=0, atol=1e-5, err_msg=f"{name} of frame {i}")
    # permutation equivariance: reversing the frame order reverses the outputs (every frame changes its stage group)
    det_r, cnt_r = eng.infer_batch(clouds[::-1])
    det_r, cnt_r = det_r.cpu().numpy(), cnt_r.cpu().numpy()
    # (the near-empty frames -- 7 points, 1 point -- are degenerate for InstanceNorm: almost constant channels, so the last bits of a
    # statistic are amplified; they get 1e-3 of the row's extent, every other frame 1e-5 -- in practice the passes are bit-identical)
    tol = [1e-3 if (n is not None and 0 < n < 100) else 1e-5 for n in sizes]
    for i in range(NB):
        assert np.array_equal(cnt_r[NB - 1 - i][:4], cnt_b[i][:4]), i
        k = int(cnt_b[i, 0])
        _assert_rows_close(det_r[NB - 1 - i, :k], det_b[i, :k], rel=tol[i])
    # the same call again gives the same detections -- 30 times: a request that is consumed before it has landed corrupts a tile of
    # one frame once in a few dozen passes (round 4: wino6_mfma's residual rows behind a wait that allowed for pending stores;
    # tools/perm_probe.py), which a single repeat almost never sees
    det_b_gpu = torch.from_numpy(det_b).cuda()
    live = torch.arange(det_b.shape[1], device="cuda")[None, :] < torch.from_numpy(cnt_b[:, 0].astype(np.int64)).cuda()[:, None]
    worst = 0.0
    for rep in range(30):
        det_2, cnt_2 = eng.infer_batch(clouds)
        assert np.array_equal(cnt_2.cpu().numpy()[:, :4], cnt_b[:, :4]), rep
        dev = (det_2[:, :, :6] - det_b_gpu[:, :, :6]).abs().amax(dim=2) / det_b_gpu[:, :, :6].abs().amax(dim=2).clamp_min(1.0)   # [frame, row]
        dev = torch.where(live, dev, torch.zeros_like(dev))   # rows behind a frame's count are not part of its result
        per_frame = dev.amax(dim=1).cpu().numpy()
        worst = max(worst, float(per_frame.max()))
        for i in range(NB):
            assert per_frame[i] <= tol[i], (rep, i, float(per_frame[i]))
    print(f"[batch repeatability] 30 repeats of the 34-frame pass: max deviation {worst:.2e} of a row's extent")
