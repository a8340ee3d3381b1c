"""GPU: the head backward at more than 9 anchors per location (csrc/train.hip: k_head_dw_wide, k_head_dx_wide behind
pp_head_backward), through the engine wrapper, on arenas, and through the autograd surface of the 10-class network.

The reference has no head with more than 9 anchors, so values are held to tests/headtrain_ref.py (float64, generic in na, pinned to
the reference's autograd goldens at na = 9 by test_headtrain_cpu.py and to torch's float64 autograd at na = 10, 20, 24 by
test_headtrain_wide_cpu.py).  Bars are the a-priori ones of test_headtrain_gpu.check_backward: a float32 sum of K products in any
order, blocked or not, is within K 2^-24 sum |a_k b_k| plus one rounding of the result (headtrain_ref.sum_bound; K = nb P for dW / db,
10 na for dX); the measured fraction must be <= 1.  Measured on an MI355X: dX 0.016 - 0.044, dW at most 0.016 (0.045 through
autograd), db at most 0.013; the unaligned call gave the aligned call's bits; the loss fell from 15.55 to 1.73 in ten Adam steps.

Configurations: nuscene_10class with a shrunk detection_range (voxel 0.16 m), its class_table cut to 5 classes (na = 10: 100 rows,
four past one 96-row block), as shipped (na = 20: 200 rows, half a 16-row tile at the end) and grown to 12 classes by copies under
new names (na = 24: 240 rows, the cap).  Maps: 8 x 6 (P = 48, one partial tile), 20 x 12 (P = 240: three full tiles and a 48-pixel
one) and, for na = 20 alone, 100 x 92 (P = 9200: 144 tiles, two per workgroup, the last one partial).

The backbone runs on grids that are multiples of 8 cells only, so what needs it (the neck scope, the fp16 forward) runs on a 16 x 16
grid (8 x 8 map) of the same 10-class network; what needs the head alone runs on the 8 x 6 map."""
import functools

import numpy as np
import pytest
import torch

from conftest import golden, load_pkg
import arena as A
import headtrain_ref as R
from test_headtrain_gpu import KEYS, check_backward
from test_train_arena_gpu import In, Out, assert_same, held
from train_common import dev

pytestmark = pytest.mark.gpu
CLASSES = {10: 5, 20: 10, 24: 12}
MAPS = {"8x6": (16, 12), "20x12": (40, 24), "100x92": (200, 184), "8x8": (16, 16)}


def wide_cfg(na, grid, max_batch):
    cfg = load_pkg("synth").load_config("nuscene_10class")
    gx, gy = MAPS[grid]
    cfg["detection_range"] = [0.0, 0.0, -3.5, 0.16 * gx, 0.16 * gy, 2.5]
    names = list(cfg["detect_class"])
    table = {n: cfg["class_table"][n] for n in names[:CLASSES[na]]}
    for i in range(CLASSES[na] - len(names)):  # copies under new names
        table[f"{names[i]}_b"] = dict(cfg["class_table"][names[i]])
    cfg["class_table"], cfg["detect_class"] = table, list(table)
    cfg["device"] = torch.device("cuda:0")
    cfg["max_batch"] = max_batch
    return cfg


def state_dict(na):
    return {k: np.asarray(v, np.float32) for k, v in load_pkg("synth").seeded_state_dict(0, num_anchor_per_loc=na).items()}


@functools.lru_cache(maxsize=None)
def engine(na, grid, max_batch=3):
    load_pkg().install()
    eng = load_pkg("engine").Engine(wide_cfg(na, grid, max_batch))
    assert eng.num_anchor_per_loc == na and (2 * eng.H, 2 * eng.W) == MAPS[grid]
    eng.load_state_dict(state_dict(na))
    return eng, R.natural_weights(state_dict(na))[0]


@functools.lru_cache(maxsize=None)
def inputs(na, grid, nb):
    """As test_head_backward_full_size: x = max(N(0, 1), 0), dY = 1e-3 N(0, 1); every frame its own data."""
    gx, gy = MAPS[grid]
    H, W = gx // 2, gy // 2
    rng = np.random.default_rng(1000 * na + H + nb)
    n = na * H * W
    x = np.maximum(rng.standard_normal((nb, 320, H, W), dtype=np.float32), 0)
    dY = [rng.standard_normal((nb, n, c), dtype=np.float32) * np.float32(1e-3) for c in (1, 7, 2)]
    return (x, *dY)


# ------------------------------------------------------------------ 1. values
CASES = [(na, grid, 3) for na in (10, 20, 24) for grid in ("8x6", "20x12")] + [(20, "100x92", 1), (20, "100x92", 2)]


@pytest.mark.parametrize("na,grid,nb", CASES, ids=[f"na{a}-{g}-nb{n}" for a, g, n in CASES])
def test_head_backward_wide(na, grid, nb):
    eng, Wn = engine(na, grid)
    check_backward(eng, *inputs(na, grid, nb), Wn, f"na {na}, map {grid}, nb {nb}")


# ------------------------------------------------------------------ 2. bits
def test_identical_calls_and_dx_skipped():
    eng, _ = engine(20, "20x12")
    args = [dev(a) for a in inputs(20, "20x12", 3)]
    g, dx = eng.head_backward(*args)
    g2, dx2 = eng.head_backward(*args)
    g3, none = eng.head_backward(*args, need_dx=False)
    assert none is None and torch.equal(dx, dx2)
    for k in KEYS:
        assert torch.equal(g[k], g2[k]) and torch.equal(g[k], g3[k]), k


# ------------------------------------------------------------------ 3. the scalar path
def shifted(a):
    """a's contents in a contiguous view that starts 4 bytes into a larger buffer"""
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device="cuda")
    off = 1 + (-buf.data_ptr() // 4) % 4  # element index with address % 16 == 4
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def test_unaligned_dbox_and_ddir():
    na, grid, nb = 20, "20x12", 3
    eng, Wn = engine(na, grid)
    x, dcls, dbox, ddir = inputs(na, grid, nb)
    g, dx = eng.head_backward(dev(x), dev(dcls), dev(dbox), dev(ddir))
    gu, dxu = eng.head_backward(dev(x), dev(dcls), shifted(dbox), shifted(ddir))
    dW, db, x64, (aW, ab, ax) = R.head_backward(x, dcls, dbox, ddir, Wn, na, bounds=True)
    P = eng.H * eng.W
    cat = lambda d, keys, w: np.concatenate([d[k].cpu().numpy().reshape(-1, w) for k in keys]).astype(np.float64)  # noqa: E731
    bW, bb, bx = R.sum_bound(nb * P, aW, dW), R.sum_bound(nb * P, ab, db), R.sum_bound(10 * na, ax, x64)
    fr = {"dW": (np.abs(cat(gu, KEYS[0::2], 320) - dW) / bW).max(), "db": (np.abs(cat(gu, KEYS[1::2], 1)[:, 0] - db) / bb).max(),
          "dX": (np.abs(dxu.cpu().numpy().astype(np.float64) - x64) / bx).max(),
          "dW against the aligned call": (np.abs(cat(gu, KEYS[0::2], 320) - cat(g, KEYS[0::2], 320)) / bW).max(),
          "dX against the aligned call": (np.abs(dxu.cpu().numpy().astype(np.float64) - dx.cpu().numpy()) / bx).max()}
    print(f"unaligned dbox / ddir: largest fraction of the summation bound {fr}")
    assert max(fr.values()) <= 1.0, fr


# ------------------------------------------------------------------ 4. memory outside the tensors
def test_arena():
    """Every argument in a guarded allocation (tests/arena.py), fills zeros, quiet NaN and +-2^40: the same output bits under every fill,
    no byte outside the outputs changed (test_train_arena_gpu.run asserts it per argument), and no output element left unwritten: the
    NaN run's outputs start as the byte 0x5A, the others' as 0xA5, so an element never stored differs between the runs; a further run
    has every pointer at an address % 16 == 4 (ddir % 16 == 8) and takes the scalar path."""
    na, grid, nb = 20, "20x12", 2
    eng, Wn = engine(na, grid)
    x, dcls, dbox, ddir = inputs(na, grid, nb)
    outs = [Out("dw_cls", (na, 320)), Out("dw_box", (7 * na, 320)), Out("dw_dir", (2 * na, 320)), Out("db_cls", (na,)), Out("db_box", (7 * na,)),
            Out("db_dir", (2 * na,))]
    args = [In("rpn_out", x), In("dcls", dcls), In("dbox", dbox), In("ddir", ddir, 8), nb] + outs + [Out("dx", x.shape), None]
    got = held(eng, "pp_head_backward", args, f"pp_head_backward na {na} {grid} nb {nb}")
    for k, t in got.items():
        assert A.pattern_free(t.cpu().numpy(), 4), k
    dW, db, x64, (aW, ab, ax) = R.head_backward(x, dcls, dbox, ddir, Wn, na, bounds=True)
    P = eng.H * eng.W
    gW = np.concatenate([got[k].cpu().numpy() for k in ("dw_cls", "dw_box", "dw_dir")]).astype(np.float64)
    gb = np.concatenate([got[k].cpu().numpy() for k in ("db_cls", "db_box", "db_dir")]).astype(np.float64)
    fr = {"dW": float((np.abs(gW - dW) / R.sum_bound(nb * P, aW, dW)).max()), "db": float((np.abs(gb - db) / R.sum_bound(nb * P, ab, db)).max()),
          "dX": float((np.abs(got["dx"].cpu().numpy().astype(np.float64) - x64) / R.sum_bound(10 * na, ax, x64)).max())}
    print(f"largest fraction of the summation bound {fr}")
    assert max(fr.values()) <= 1.0, fr
    no_dx = held(eng, "pp_head_backward", args[:-2] + [None, None], "pp_head_backward, dx NULL", odd=False)
    assert_same(no_dx, {k: got[k] for k in no_dx}, "pp_head_backward: dx NULL")


# ------------------------------------------------------------------ 5 / 6. the 10-class network
def gt_frames(cfg):
    """Two frames of ground truth inside the 2.56 m x 1.92 m the small maps cover: six classes, four per frame.  On the host
    (assign_ref.assign_frame over engine.build_anchor_tables) they give 8 and 19 positives on the 8 x 6 map and on the 8 x 8 map."""
    names, tab = list(cfg["detect_class"]), cfg["class_table"]

    def box(n, x, y, r):
        return [x, y, -1.0, *tab[n]["sizes"][0], r]

    frames = [[("pedestrian", 0.5, 0.5, 0.3), ("traffic_cone", 1.9, 1.3, 0.0), ("bicycle", 1.3, 1.0, 0.1), ("barrier", 2.2, 0.9, 1.5)],
              [("motorcycle", 1.2, 0.6, 1.6), ("pedestrian", 2.0, 1.5, 0.0), ("car", 1.3, 1.0, 0.05), ("traffic_cone", 0.4, 1.5, 0.7)]]
    assert len({b[0] for f in frames for b in f}) >= 4
    return [(np.array([names.index(b[0]) + 1 for b in f], np.int32), np.array([box(*b) for b in f], np.float32)) for f in frames]


def network(grid, precision=None, sd=None):
    """The 10-class network on a small grid, with LossGenerator and the targets AnchorAssigner.assign_batch gives for gt_frames."""
    load_pkg().install()
    cfg = wide_cfg(20, grid, 4)
    load_pkg("framework.voxel_generator").VoxelGenerator(cfg)
    net = load_pkg("networks.pointpillars8_shared").PointPillars(cfg)
    net.profile_stages = False
    if precision:
        net.precision(precision)
    net.load_state_dict(state_dict(20) if sd is None else sd)
    eng = net._eng
    assert eng.num_anchor_per_loc == 20
    asg = load_pkg("framework.anchor_assigner").AnchorAssigner(cfg)
    labels, tgt, _, dirt = asg.assign_batch(gt_frames(cfg), torch.ones((2, eng.A), dtype=torch.uint8, device=eng.device))
    assert all(int((labels[f] > 0).sum()) > 0 for f in range(2)), "both frames have positives"
    ex = {"labels": labels, "bbox_targets": tgt, "dir_targets": dirt}
    return net, cfg, load_pkg("framework.loss_generator").LossGenerator(cfg), ex


def pillars(eng, gx, gy):
    """Two frames of pillars on a gx x gy grid, collated as the loader does."""
    rng = np.random.default_rng(4)
    frames = []
    for f in range(2):
        n = 30 + 10 * f
        cells = rng.choice(gx * gy, n, replace=False)
        coors = np.stack([cells // gy, cells % gy, np.zeros(n, np.int64)], 1).astype(np.int32)
        vox = rng.standard_normal((n, eng.T, eng.F)).astype(np.float32)
        frames.append(dict(voxels=vox, coordinates=coors, num_points_per_voxel=rng.integers(1, eng.T + 1, n).astype(np.int32)))
    utils = load_pkg("framework.utils")
    return utils.example_convert_to_torch(utils.merge_second_batch(frames))


def test_autograd_surface_and_training():
    """net.train(); loss.backward() on the 10-class network.  The gradients are the engine's own calls bit for bit.  Against float64
    they are held in the two steps the project holds each call in: the device's dY to headtrain_ref.loss_grad at the device's float32
    logits, bar 4 x ref32_dev x max |g64| (the reference's own float32 deviation of that gradient, from the headtrain_small fixture:
    the bar of test_headtrain_gpu and test_train_arena_gpu); the parameter and input gradients to headtrain_ref.head_backward of that
    dY, which is exact in float32, under the summation bound."""
    net, cfg, lg, ex = network("8x6")
    eng, na = net._eng, 20
    rng = np.random.default_rng(7)
    x_np = np.maximum(rng.standard_normal((2, 320, eng.H, eng.W), dtype=np.float32), 0)
    x = dev(x_np)
    plain = net.heads(x)
    net.train()
    assert [k for k, _ in net.named_parameters()] == list(KEYS)
    xg = x.clone().requires_grad_(True)
    preds = net.heads(xg)
    assert all(torch.equal(preds[k], plain[k]) for k in plain)
    loss = lg.generate(preds, ex)["loss"]
    net.zero_grad()
    loss.backward()
    dY = eng.target_loss_grad(plain["cls_preds"], plain["box_preds"], plain["dir_preds"], ex["labels"], ex["bbox_targets"], ex["dir_targets"])
    gr, dx = eng.head_backward(x, *dY)
    for k, p in net.named_parameters():
        assert p.grad is not None and torch.equal(p.grad, gr[k].reshape(p.shape)), k
    assert torch.equal(xg.grad, dx)
    # float64, step one: the loss gradient at the device's logits
    g = golden("headtrain_small")
    lab, tgt, dirt = (ex[k].cpu().numpy() for k in ("labels", "bbox_targets", "dir_targets"))
    want = R.loss_grad(*[plain[k].cpu().numpy() for k in ("cls_preds", "box_preds", "dir_preds")], lab, tgt, dirt)
    for n, t, w in zip(("dcls", "dbox", "ddir"), dY, want):
        err, bar = np.abs(t.cpu().numpy().astype(np.float64).reshape(w.shape) - w).max(), 4.0 * float(g["ref32_dev_" + n]) * np.abs(w).max()
        print(f"{n}: max err {err:.3e}, bar {bar:.3e} ({err / bar:.2f} of it)")
        assert err <= bar and np.abs(w).max() > 0, n
    # step two: the head backward of that dY
    Wn, _ = R.natural_weights(state_dict(na))
    dY_np = [t.cpu().numpy().reshape(2, eng.A, c) for t, c in zip(dY, (1, 7, 2))]
    dW, db, x64, (aW, ab, ax) = R.head_backward(x_np, *dY_np, Wn, na, bounds=True)
    params = dict(net.named_parameters())
    gW = np.concatenate([params[k].grad.cpu().numpy().reshape(-1, 320) for k in KEYS[0::2]]).astype(np.float64)
    gb = np.concatenate([params[k].grad.cpu().numpy() for k in KEYS[1::2]]).astype(np.float64)
    P = eng.H * eng.W
    fr = {"dW": float((np.abs(gW - dW) / R.sum_bound(2 * P, aW, dW)).max()), "db": float((np.abs(gb - db) / R.sum_bound(2 * P, ab, db)).max()),
          "dX": float((np.abs(xg.grad.cpu().numpy().astype(np.float64) - x64) / R.sum_bound(10 * na, ax, x64)).max())}
    print(f"largest fraction of the summation bound {fr}")
    assert max(fr.values()) <= 1.0 and np.abs(dW).max() > 0, fr
    # ten Adam steps
    optim = load_pkg("framework.optim")
    opt = optim.Adam(net.parameters(), lr=1e-3)
    losses = []
    for _ in range(10):
        loss = lg.generate(net.heads(x), ex)["loss"]
        opt.zero_grad()
        loss.backward()
        optim.clip_grad_norm_(list(net.parameters()), 10.0)
        opt.step()
        losses.append(float(loss.detach()))
    losses.append(float(lg.generate(net.heads(x), ex)["loss"].detach()))
    print("loss before each step and after the tenth:", " ".join(f"{v:.5f}" for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < 0.5 * losses[0], losses
    # the stepped head in eval mode
    net.eval()
    got = net.heads(x)
    sd = net.state_dict()
    Wn, bn = R.natural_weights(sd)
    assert np.abs(Wn - R.natural_weights(state_dict(na))[0]).max() > 1e-3
    for k, w in zip(("cls_preds", "box_preds", "dir_preds"), R.head_forward(x_np.astype(np.float64), Wn, bn, na)):
        np.testing.assert_allclose(got[k].cpu().numpy(), w, rtol=0, atol=2e-5)


def test_neck_scope():
    """train(scope="neck") on the 10-class network (8 x 8 map: the backbone's smallest grid): one loss.backward() reaches the three
    upsamplers through the wide head backward's dX; finite, non-zero, and the same bits in a second run."""
    net, cfg, lg, ex = network("8x8")
    eng = net._eng
    example = pillars(eng, 16, 16)
    neck = load_pkg("networks.pointpillars8_shared").NECK_KEYS
    net.train(scope="neck")
    runs = []
    for _ in range(2):
        loss = lg.generate(net(example), ex)["loss"]
        net.zero_grad()
        loss.backward()
        params = dict(net.named_parameters())
        runs.append({k: params[k].grad.clone() for k in neck + tuple(KEYS)})
    for k in neck:
        assert torch.isfinite(runs[0][k]).all() and float(runs[0][k].abs().max()) > 0, k
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_fp16_forward_one_step():
    """train(forward_precision="fp16"), one Adam step: pp_update_head_weights_mp and its refresh of the natural-order copy at na = 20.
    In eval mode the network then equals a fresh one loaded with the stepped state_dict() in precision("fp16"), bit for bit; and a
    further head backward's dX equals the one an fp32 engine computes from the stepped weights (the copy is fp32 in every mode)."""
    net, cfg, lg, ex = network("8x8")
    eng = net._eng
    example = pillars(eng, 16, 16)
    net.train(forward_precision="fp16")
    assert eng.effective_precision() == "fp16"
    opt = load_pkg("framework.optim").Adam(net.parameters(), lr=1e-3)
    loss = lg.generate(net(example), ex)["loss"]
    opt.zero_grad()
    loss.backward()
    opt.step()
    net.eval()
    got = net(example)
    sd = net.state_dict()
    assert np.abs(np.asarray(sd[KEYS[0]]).reshape(-1) - state_dict(20)[KEYS[0]].reshape(-1)).max() > 1e-4
    other, _, _, _ = network("8x8", precision="fp16", sd=sd)
    assert other._eng.layer_tilings() == eng.layer_tilings() and other._eng.effective_precision() == "fp16"
    want = other(example)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    plain = load_pkg("engine").Engine(wide_cfg(20, "8x8", 4))
    plain.load_state_dict({k: np.asarray(v, np.float32) for k, v in sd.items()})
    x, dcls, dbox, ddir = (dev(a) for a in inputs(20, "8x8", 2))
    _, dx = eng.head_backward(x, dcls, dbox, ddir)
    _, dx32 = plain.head_backward(x, dcls, dbox, ddir)
    assert torch.equal(dx, dx32)


# ------------------------------------------------------------------ 7. the cap
def test_more_than_24_anchors_refused():
    """5 classes x 3 sizes x 2 rotations = 30 anchors per location: the forward takes them, pp_head_backward names its cap."""
    cfg = wide_cfg(10, "8x6", 2)
    for t in cfg["class_table"].values():
        t["sizes"] = [list(t["sizes"][0]), [v * 1.5 for v in t["sizes"][0]], [v * 2.0 for v in t["sizes"][0]]]
    load_pkg().install()
    eng = load_pkg("engine").Engine(cfg)
    assert eng.num_anchor_per_loc == 30
    eng.load_state_dict(state_dict(30))
    H, W = eng.H, eng.W
    x = torch.zeros((1, 320, H, W), device="cuda")
    cls, box, dr = eng.head(x)
    assert cls.shape == (1, 30 * H * W, 1)
    with pytest.raises(RuntimeError, match="more than 24 anchors per location"):
        eng.head_backward(x, torch.zeros_like(cls), torch.zeros_like(box), torch.zeros_like(dr))
    ok, _ = engine(24, "8x6")  # and the cap itself is accepted (test_head_backward_wide holds its values)
    assert ok.num_anchor_per_loc == 24
