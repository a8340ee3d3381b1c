"""GPU: anchor target assignment, detection loss and metric counts (assign.hip) against the reference's goldens
(tests/golden/make_assign_goldens.py) and the CPU restatements pinned to them (tests/assign_ref.py)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden, load_pkg
import assign_ref
from test_assign_cpu import golden_frame

pytestmark = pytest.mark.gpu

MAXB = 32


def make_cfg(name, max_batch=MAXB):
    cfg = load_pkg("synth").load_config(name)
    cfg["device"] = torch.device("cuda:0")
    cfg["max_batch"] = max_batch
    return cfg


@pytest.fixture(scope="module")
def env():
    cfg = make_cfg("eight_20cm")
    eng = load_pkg("engine").engine_for(cfg)
    return cfg, eng


def ulp_diff(a, b):
    ai = a.view(np.int32).astype(np.int64)
    bi = b.view(np.int32).astype(np.int64)
    return np.abs(ai - bi)


def check_frame(eng, r, labels, tgt, dirt, what):
    lab = r[0].cpu().numpy()
    t = r[1].cpu().numpy()
    ow = r[2].cpu().numpy()
    d = r[3].cpu().numpy()
    assert np.array_equal(lab, labels), what
    assert np.array_equal(ow, (labels > 0).astype(np.float32)), what
    assert np.array_equal(d, dirt), what
    pos = labels > 0
    assert np.array_equal(t[~pos], tgt[~pos]), what
    for k in (0, 1, 2, 6):
        assert np.array_equal(t[pos, k], tgt[pos, k]), f"{what}: code {k}"
    for k in (3, 4, 5):
        assert ulp_diff(t[pos, k], tgt[pos, k]).max(initial=0) <= 2, f"{what}: code {k}"


def gt_tensors(frames, dev):
    box = torch.from_numpy(np.concatenate([np.asarray(b, np.float32).reshape(-1, 7) for _, b in frames])).to(dev)
    cls = torch.from_numpy(np.concatenate([np.asarray(c, np.int32).reshape(-1) for c, _ in frames])).to(dev)
    off = np.concatenate([[0], np.cumsum([len(c) for c, _ in frames])]).tolist()
    return box, cls, off


def test_assign_golden_frames_bit_exact(env):
    cfg, eng = env
    g = golden("assign_eight_20cm")
    for f in range(int(g["nframes"])):
        mask, gt, gc, labels, tgt, dirt = golden_frame(g, f, eng.A)
        box, cls, off = gt_tensors([(gc, gt)], eng.device)
        r = eng.assign_targets(torch.from_numpy(mask.astype(np.uint8)).to(eng.device).reshape(1, -1), box, cls, off)
        check_frame(eng, [x[0] for x in r], labels, tgt, dirt, f"golden frame {f}")


def test_device_chain_on_golden_cloud(env):
    cfg, eng = env
    g = golden("assign_eight_20cm")
    pts = load_pkg("synth").lidar_cloud("eight_20cm", seed=int(g["cloud_seed"]))
    _, coors, _, num = eng.voxelize(torch.from_numpy(pts).to(eng.device))
    mask = eng.anchor_mask(coors, num)
    mask_g, gt, gc, labels, tgt, dirt = golden_frame(g, 0, eng.A)
    assert np.array_equal(mask.cpu().numpy().astype(bool), mask_g)
    box, cls, off = gt_tensors([(gc, gt)], eng.device)
    r = eng.assign_targets(mask.reshape(1, -1), box, cls, off)
    check_frame(eng, [x[0] for x in r], labels, tgt, dirt, "device chain")


def random_frames(rng, eng, n, cfg):
    ncls = eng.cfg.num_classes
    lo, hi = np.asarray(cfg["detection_range"][:2], np.float32), np.asarray(cfg["detection_range"][3:5], np.float32)
    frames, masks = [], []
    for i in range(n):
        k = [0, 1, 7, 25, 3][i % 5]
        xy = rng.uniform(lo * 0.9, hi * 0.9, (k, 2))
        dims = rng.uniform([0.6, 0.5, 1.4], [6.0, 2.6, 3.0], (k, 3))
        r = rng.uniform(-np.pi, np.pi, (k, 1))
        b = np.concatenate([xy, rng.uniform(-2, 0, (k, 1)), dims, r], 1).astype(np.float32)
        frames.append((rng.integers(1, ncls + 1, k).astype(np.int32), b))
        masks.append(rng.random(eng.A) < [0.0, 1.0, 0.3, 0.05, 0.6][i % 5])
    return frames, np.stack(masks).astype(np.uint8)


def test_batched_equals_single_frame_calls(env):
    cfg, eng = env
    rng = np.random.default_rng(3)
    frames, masks = random_frames(rng, eng, MAXB, cfg)
    box, cls, off = gt_tensors(frames, eng.device)
    mk = torch.from_numpy(masks).to(eng.device)
    rb = eng.assign_targets(mk, box, cls, off)
    assert len({len(c) for c, _ in frames}) == 5 and all(masks[f].any() for f in range(MAXB) if f % 5)
    for f in range(MAXB):  # every frame: box counts 0, 1, 7, 25, 3 and mask densities 0 .. 1, both halves of the batch
        b1, c1, o1 = gt_tensors([frames[f]], eng.device)
        r1 = eng.assign_targets(mk[f:f + 1].contiguous(), b1, c1, o1)
        for x, y in zip(rb, r1):
            assert torch.equal(x[f], y[0]), f"frame {f}"


@pytest.mark.parametrize("name", ["eight_20cm", "ntusl_10cm", "nuscene", "nuscene_10class"])
def test_random_boxes_against_restatement(name):
    cfg = make_cfg(name, max_batch=4)
    eng = load_pkg("engine").engine_for(cfg)
    rng = np.random.default_rng(11)
    frames, masks = random_frames(rng, eng, 4, cfg)
    box, cls, off = gt_tensors(frames, eng.device)
    r = eng.assign_targets(torch.from_numpy(masks).to(eng.device), box, cls, off)
    names = list(eng.class_masks)
    tm = [eng.class_table[n].get("matched_threshold", 0.6) for n in names]
    tu = [eng.class_table[n].get("unmatched_threshold", 0.45) for n in names]
    for f in range(4):
        ref = assign_ref.assign_frame(eng.anchors_np, eng.anchors_bv, list(eng.class_masks.values()), tm, tu, frames[f][1], frames[f][0],
                                      masks[f])
        assert np.array_equal(r[0][f].cpu().numpy(), ref["labels"]), f"{name} frame {f}"
        assert np.array_equal(r[3][f].cpu().numpy(), ref["dir_targets"]), f"{name} frame {f}"


def golden_loss_inputs(eng):
    import sys
    sys.path.insert(0, GOLDEN)
    import make_assign_goldens as mk
    from make_goldens import sha
    g = golden("assign_eight_20cm")
    lg = golden("loss_eight_20cm")
    frames = [int(f) for f in lg["frames"]]
    cls, box, dr = mk.logits(int(lg["seed"]), eng.A, len(frames))
    assert sha(cls, box, dr) == str(lg["logits_sha"])
    gf = [golden_frame(g, f, eng.A) for f in frames]
    return lg, cls, box, dr, gf


def test_target_loss_golden(env):
    cfg, eng = env
    lg, cls, box, dr, gf = golden_loss_inputs(eng)
    d = eng.device
    labels = torch.from_numpy(np.stack([x[3] for x in gf])).to(d)
    tgt = torch.from_numpy(np.stack([x[4] for x in gf])).to(d)
    dirt = torch.from_numpy(np.stack([x[5] for x in gf])).to(d)
    args = [torch.from_numpy(a).to(d) for a in (cls, box, dr)]
    t1 = eng.target_loss(*args, labels, tgt, dirt)
    t2 = eng.target_loss(*args, labels, tgt, dirt)
    assert torch.equal(t1, t2)
    lgm = load_pkg("framework.loss_generator")
    got = lgm.combine_terms(t1.cpu().numpy())
    for k, v in zip(lg["keys"], lg["values"]):
        assert got[str(k)] == pytest.approx(float(v), rel=1e-5), k
    counts = t1.cpu().numpy()[:, 5:21].sum(0).reshape(4, 4).astype(np.int64)
    assert np.array_equal(counts, lg["counts"])
    # the drop-ins on the same inputs
    gen = lgm.LossGenerator(cfg).generate({"cls_preds": args[0], "box_preds": args[1], "dir_preds": args[2]},
                                          {"labels": labels.cpu().numpy(), "bbox_targets": tgt.cpu().numpy(), "dir_targets": dirt.cpu().numpy()})
    assert set(gen) == set(lgm.KEYS) and all(v.dim() == 0 for v in gen.values())
    for k, v in zip(lg["keys"], lg["values"]):
        assert float(gen[str(k)]) == pytest.approx(float(v), rel=1e-5), k
    Metric = load_pkg("framework.metrics").Metric
    m = Metric(cfg)
    m.update(labels.cpu().numpy(), args[0])
    ref_str = ""
    prec = [c[0] / max(c[0] + c[2], 1) for c in lg["counts"]]
    rec = [c[0] / max(c[0] + c[3], 1) for c in lg["counts"]]
    for i, t in enumerate([0.1, 0.3, 0.5, 0.7]):
        ref_str += "@%.2f prec:%.5f, rec:%.5f  " % (t, prec[i], rec[i])
    assert str(m) == ref_str
    m.clear()
    assert float(m.rec_count.sum()) == 0


@pytest.fixture(scope="module")
def batch8(env):
    cfg, eng = env
    synth = load_pkg("synth")
    eng.load_state_dict(synth.seeded_state_dict(0, cls_bias=-3.0))
    clouds = [synth.lidar_cloud("eight_20cm", seed=100 + i) for i in range(20)]
    rng = np.random.default_rng(7)
    gts = []
    for i, c in enumerate(clouds):
        k = [0, 4, 12, 2][i % 4]
        p = c[rng.integers(0, c.shape[0], k)]
        b = np.concatenate([p[:, :2], np.full((k, 1), -1.0), rng.uniform([0.7, 0.6, 1.5], [5, 2.2, 2.0], (k, 3)),
                            rng.uniform(-np.pi, np.pi, (k, 1))], 1).astype(np.float32)
        gts.append((rng.integers(1, 4, k).astype(np.int32), b))
    return clouds, gts


def test_batch_loss_equals_assign_plus_target_loss(env, batch8):
    cfg, eng = env
    clouds, gts = batch8
    d = eng.device
    eng.infer_batch([torch.from_numpy(c).to(d) for c in clouds[:8]])
    box, cls, off = gt_tensors(gts[:8], d)
    tb = eng.batch_loss(box, cls, off, 8)
    masks = torch.stack([eng.fetch(f, "mask") for f in range(8)])
    lab, tgt, ow, dirt = eng.assign_targets(masks, box, cls, off)
    c = torch.stack([eng.fetch(f, "cls") for f in range(8)])
    b = torch.stack([eng.fetch(f, "box") for f in range(8)])
    dr = torch.stack([eng.fetch(f, "dir") for f in range(8)])
    tl = eng.target_loss(c, b, dr, lab, tgt, dirt)
    assert torch.equal(tb, tl)
    assert torch.equal(eng.batch_loss(box, cls, off, 8), tb)
    for f in range(8):
        ref = assign_ref.loss_terms(c[f].cpu(), b[f].cpu(), dr[f].cpu(), lab[f].cpu(), tgt[f].cpu(), dirt[f].cpu())
        t = tb[f].cpu().numpy()
        assert t[0] == ref["npos"]
        for i, k in enumerate(("loc", "cls_pos", "cls_neg", "dir")):
            assert t[1 + i] == pytest.approx(ref[k], rel=1e-5, abs=1e-12), (f, k)
        assert np.array_equal(t[5:21].reshape(4, 4).astype(np.int64), ref["counts"])


def test_assign_drop_in_numpy_and_sequence_loss(env, batch8):
    cfg, eng = env
    clouds, gts = batch8
    load_pkg("framework.voxel_generator").VoxelGenerator(cfg)  # fills grid_size / detection_offset, as in the reference's train.py
    aa = load_pkg("framework.anchor_assigner").AnchorAssigner(cfg)
    g = golden("assign_eight_20cm")
    mask, gt, gc, labels, tgt, dirt = golden_frame(g, 0, eng.A)
    out = aa.assign(gc, gt, mask)
    assert all(isinstance(x, np.ndarray) for x in out)
    assert [x.dtype for x in out] == [np.int32, np.float32, np.float32, np.int32]
    assert [x.shape for x in out] == [(eng.A,), (eng.A, 7), (eng.A,), (eng.A,)]
    assert np.array_equal(out[0], labels) and np.array_equal(out[3], dirt)
    dev = aa.assign(torch.from_numpy(gc).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(mask).cuda())
    assert all(x.is_cuda for x in dev) and torch.equal(dev[0].cpu(), torch.from_numpy(labels))
    kio = load_pkg("kitti_io")
    losses, metric = kio.sequence_loss(cfg, clouds, gts, batch=8)
    assert len(losses) == 20
    lgm = load_pkg("framework.loss_generator")
    Metric = load_pkg("framework.metrics").Metric
    m2 = Metric(cfg)
    per = []
    for i0 in range(0, 20, 8):
        nb = min(8, 20 - i0)
        eng.infer_batch([torch.from_numpy(c).to(eng.device) for c in clouds[i0:i0 + nb]])
        box, cls, off = gt_tensors(gts[i0:i0 + nb], eng.device)
        t = eng.batch_loss(box, cls, off, nb).cpu().numpy()
        per += [lgm.combine_terms(t[f:f + 1]) for f in range(nb)]
        m2.update_counts(t)
    assert losses == per
    assert str(metric) == str(m2)


def test_bad_arguments_raise_before_launch(env):
    cfg, eng = env
    d = eng.device
    mask = torch.ones((1, eng.A), dtype=torch.uint8, device=d)
    box = torch.zeros((2, 7), dtype=torch.float32, device=d)
    for bad in ([0, 1], [1, 4]):
        with pytest.raises(ValueError):
            eng.assign_targets(mask, box, torch.tensor(bad, dtype=torch.int32, device=d), [0, 2])
    ok_cls = torch.ones(2, dtype=torch.int32, device=d)
    with pytest.raises(ValueError):
        eng.assign_targets(torch.ones((MAXB + 1, eng.A), dtype=torch.uint8, device=d), box, ok_cls, [0] * MAXB + [1, 2])
    with pytest.raises(ValueError):
        eng.assign_targets(torch.ones((2, eng.A), dtype=torch.uint8, device=d), box, ok_cls, [0, 2, 1])
    _lib = load_pkg("_lib")
    G = _lib.PP_ASSIGN_MAX_GT + 1
    with pytest.raises(ValueError):
        eng.assign_targets(mask, torch.zeros((G, 7), dtype=torch.float32, device=d), torch.ones(G, dtype=torch.int32, device=d), [0, G])
    # the C ABI's own checks (host side, nothing launched)
    lib = eng.lib
    off = (ctypes.c_int32 * 3)(0, 2, 1)
    rc = lib.pp_batch_loss(eng.ctx, ctypes.c_void_p(box.data_ptr()), ctypes.c_void_p(ok_cls.data_ptr()), off, 2, ctypes.c_void_p(box.data_ptr()), None)
    assert rc == 1
    off = (ctypes.c_int32 * 2)(0, G)
    rc = lib.pp_batch_loss(eng.ctx, ctypes.c_void_p(box.data_ptr()), ctypes.c_void_p(ok_cls.data_ptr()), off, 1, ctypes.c_void_p(box.data_ptr()), None)
    assert rc == 1
    rc = lib.pp_target_loss(eng.ctx, *([ctypes.c_void_p(box.data_ptr())] * 6), MAXB + 1, ctypes.c_void_p(box.data_ptr()), None)
    assert rc == 1
    torch.cuda.synchronize()


def test_label_order_with_matched_below_unmatched(env):
    """The reference's order (anchor_assigner.py:381-392): bg (< unmatched) overwrites pos (>= matched), forced last."""
    cfg, eng = env
    g = golden("assign_eight_20cm")
    mask, gt, gc, *_ = golden_frame(g, 0, eng.A)
    tm, tu = [0.3, 0.05, 0.2], [0.45, 0.3, 0.25]
    names = list(eng.class_masks)
    try:
        eng.set_assign_thresholds(tm, tu)
        box, cls, off = gt_tensors([(gc, gt)], eng.device)
        r = eng.assign_targets(torch.from_numpy(mask.astype(np.uint8)).to(eng.device).reshape(1, -1), box, cls, off)
        ref = assign_ref.assign_frame(eng.anchors_np, eng.anchors_bv, list(eng.class_masks.values()), tm, tu, gt, gc, mask)
        assert np.array_equal(r[0][0].cpu().numpy(), ref["labels"])
        mid = np.zeros(eng.A, bool)
        for c, (s_, e_) in enumerate(eng.class_masks.values()):
            mx = ref["max"][s_:e_]
            mid[s_:e_] = (mx >= tm[c]) & (mx < tu[c]) & ~ref["forced"][s_:e_]
        assert mid.any() and (ref["labels"][mid] == 0).all()
    finally:
        eng.set_assign_thresholds([eng.class_table[n].get("matched_threshold", 0.6) for n in names],
                                  [eng.class_table[n].get("unmatched_threshold", 0.45) for n in names])


def test_batch_loss_refuses_frames_beyond_last_pass(env, batch8):
    cfg, eng = env
    clouds, gts = batch8
    d = eng.device
    eng.infer_batch([torch.from_numpy(c).to(d) for c in clouds[:3]])
    box, cls, off = gt_tensors(gts[:4], d)
    with pytest.raises(RuntimeError, match="last inference pass"):
        eng.batch_loss(box, cls, off, 4)
    box, cls, off = gt_tensors(gts[:3], d)
    assert eng.batch_loss(box, cls, off, 3).shape == (3, load_pkg("_lib").PP_LOSS_TERMS)


def test_metric_without_config_matches_counts(env):
    cfg, eng = env
    lg, cls, box, dr, gf = golden_loss_inputs(eng)
    labels = np.stack([x[3] for x in gf])
    m = load_pkg("framework.metrics").Metric()
    m.update(labels, torch.from_numpy(cls).to(eng.device))
    m2 = load_pkg("framework.metrics").Metric()
    m2.update_counts(lg["counts"])
    assert str(m) == str(m2)


def test_timings_32_frame_batch(env, batch8):
    """Kernel time per call from HIP events around back-to-back C calls (arguments built and checked beforehand)."""
    cfg, eng = env
    clouds, gts = batch8
    d = eng.device
    lib, ctx, st = eng.lib, eng.ctx, torch.cuda.current_stream().cuda_stream
    batch = [torch.from_numpy(clouds[i % len(clouds)]).to(d) for i in range(MAXB)]
    gt32 = [gts[i % len(gts)] for i in range(MAXB)]
    box, cls, off = gt_tensors(gt32, d)
    offh = (ctypes.c_int32 * (MAXB + 1))(*off)
    det, cnt = eng.infer_batch(batch)
    masks = torch.stack([eng.fetch(f, "mask") for f in range(MAXB)])
    c = torch.stack([eng.fetch(f, "cls") for f in range(MAXB)])
    b = torch.stack([eng.fetch(f, "box") for f in range(MAXB)])
    dr = torch.stack([eng.fetch(f, "dir") for f in range(MAXB)])
    lab = torch.empty((MAXB, eng.A), dtype=torch.int32, device=d)
    tgt = torch.empty((MAXB, eng.A, 7), dtype=torch.float32, device=d)
    ow = torch.empty((MAXB, eng.A), dtype=torch.float32, device=d)
    dirt = torch.empty((MAXB, eng.A), dtype=torch.int32, device=d)
    terms = torch.empty((MAXB, 21), dtype=torch.float64, device=d)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def timed(fn, n=10):
        assert fn() == 0
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / n

    t_assign = timed(lambda: lib.pp_assign_targets(ctx, P(masks), P(box), P(cls), offh, MAXB, P(lab), P(tgt), P(ow), P(dirt), st))
    t_loss = timed(lambda: lib.pp_target_loss(ctx, P(c), P(b), P(dr), P(lab), P(tgt), P(dirt), MAXB, P(terms), st))
    eng.infer_batch(batch, det, cnt)
    t_fused = timed(lambda: lib.pp_batch_loss(ctx, P(box), P(cls), offh, MAXB, P(terms), st))
    print(f"\n32-frame batch, {off[-1]} boxes (kernel time, HIP events): pp_assign_targets {t_assign:.3f} ms, pp_target_loss {t_loss:.3f} ms, "
          f"pp_batch_loss {t_fused:.3f} ms")
