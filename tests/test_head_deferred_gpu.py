"""Deferred head (-m gpu): a pass computes the head's cls rows for every pixel and the box / dir logits of the selected candidates
only.  Everything here is an equality: the candidate head runs the full head's MFMA arithmetic on the same weight image, so
detections, counts and (after lazy materialisation) the full tensors are bit-identical to the full-head mode."""
import numpy as np
import pytest
import torch

from conftest import load_pkg

pytestmark = pytest.mark.gpu

MAXB = 34  # crosses PP_GROUP = 32


def make_cfg(synth, name, **over):
    cfg = synth.load_config(name)
    cfg.update(over)
    cfg["device"] = torch.device("cuda:0")
    return cfg


@pytest.fixture(scope="module")
def eight(synth):
    eng = load_pkg("engine").Engine(make_cfg(synth, "eight_20cm"), max_batch=MAXB)
    clouds = [torch.from_numpy(synth.lidar_cloud("eight_20cm", seed=1000 + i)).cuda() for i in range(MAXB)]
    return eng, clouds


def both_modes(eng, clouds, nms_mode):
    """(det, cnt) of one pass in deferred mode and in full-head mode, as host-independent clones."""
    out = []
    for on in (True, False):
        eng.set_head_defer(on)
        assert eng.head_defer_active() == on
        det, cnt = eng.infer_batch(clouds, nms_mode=nms_mode)
        torch.cuda.synchronize()
        out.append((det.clone(), cnt.clone()))
    eng.set_head_defer(True)
    return out


def assert_same(a, b, what):
    (da, ca), (db, cb) = a, b
    assert torch.equal(ca, cb), what + ": counts differ"
    for f in range(ca.shape[0]):
        n = int(ca[f, 0])
        assert torch.equal(da[f, :n], db[f, :n]), f"{what}: detections of frame {f} differ"
    return int(ca[:, 0].sum())


@pytest.mark.parametrize("nms_mode", [0, 1])
@pytest.mark.parametrize("cls_bias", [None, -4.6])
@pytest.mark.parametrize("nframes", [1, 5, MAXB])  # 1: the candidate head finalises the fp64 statistics itself
def test_deferred_equals_full(eight, synth, nframes, cls_bias, nms_mode):
    eng, clouds = eight
    eng.load_state_dict(synth.seeded_state_dict(0, cls_bias=cls_bias))
    d, f = both_modes(eng, clouds[:nframes], nms_mode)
    total = assert_same(d, f, f"{nframes} frames, cls_bias {cls_bias}, nms {nms_mode}")
    print(f"[head deferred] {nframes} frames cls_bias={cls_bias} nms={nms_mode}: {total} detections, equal")
    assert total > 0


@pytest.mark.parametrize("nms_mode", [0, 1])
def test_no_candidates(eight, synth, nms_mode):
    eng, clouds = eight
    eng.load_state_dict(synth.seeded_state_dict(0, cls_bias=-30.0))
    d, f = both_modes(eng, clouds[:3], nms_mode)
    assert assert_same(d, f, "cls_bias -30") == 0
    assert int(d[1].abs().sum()) == 0


@pytest.mark.parametrize("nms_mode", [0, 1])
def test_all_equal_scores_take_the_radix_fallback(eight, synth, nms_mode):
    eng, clouds = eight
    sd = synth.seeded_state_dict(0)
    sd["heads.conv_cls.weight"] = torch.zeros_like(torch.as_tensor(sd["heads.conv_cls.weight"]))
    sd["heads.conv_cls.bias"] = torch.zeros_like(torch.as_tensor(sd["heads.conv_cls.bias"]))  # sigmoid(0) = 0.5 >= 0.05 everywhere
    eng.load_state_dict(sd)
    d, f = both_modes(eng, clouds[:3], nms_mode)
    assert assert_same(d, f, "all-equal scores") > 0
    # the fallback is what ran: every masked-in anchor of a class passes the threshold with ONE score, so the short list (4096 keys)
    # overflows wherever a class has more masked-in anchors than that
    for fr in range(3):
        mask = eng.fetch(fr, "mask").cpu().numpy().astype(bool)
        per_class = [int(mask[s:e].sum()) for s, e in eng.class_masks.values()]
        print(f"[head deferred] all-equal scores, frame {fr}: masked-in anchors per class {per_class}")
        assert min(per_class) > 4096, per_class
    assert torch.equal(eng.fetch(1, "cls"), torch.zeros(eng.A, device=eng.device))


def some_gt(eng, cfg, nb):
    rng = np.random.default_rng(5)
    lo, hi = np.asarray(cfg["detection_range"][:2], np.float32), np.asarray(cfg["detection_range"][3:5], np.float32)
    boxes, classes, off = [], [], [0]
    for i in range(nb):
        k = [3, 0, 7][i % 3]
        xy = rng.uniform(lo * 0.8, hi * 0.8, (k, 2))
        dims = rng.uniform([0.6, 0.5, 1.4], [6.0, 2.6, 3.0], (k, 3))
        boxes.append(np.concatenate([xy, rng.uniform(-2, 0, (k, 1)), dims, rng.uniform(-np.pi, np.pi, (k, 1))], 1).astype(np.float32))
        classes.append(rng.integers(1, eng.cfg.num_classes + 1, k).astype(np.int32))
        off.append(off[-1] + k)
    return torch.from_numpy(np.concatenate(boxes)).to(eng.device), torch.from_numpy(np.concatenate(classes)).to(eng.device), off


@pytest.mark.parametrize("nframes", [1, 5])
def test_fetch_and_batch_loss_materialise(eight, synth, nframes):
    eng, clouds = eight
    cfg = synth.load_config("eight_20cm")
    eng.load_state_dict(synth.seeded_state_dict(0, cls_bias=-4.6))
    box, cls, off = some_gt(eng, cfg, nframes)
    got = {}
    for on in (False, True):
        eng.set_head_defer(on)
        eng.infer_batch(clouds[:nframes])
        terms = eng.batch_loss(box, cls, off, nframes).clone()  # first consumer of the stale tensors in deferred mode
        eng.infer_batch(clouds[:nframes])
        got[on] = ([eng.fetch(f, w).clone() for f in range(nframes) for w in ("box", "dir", "cls")], terms)
    for a, b in zip(got[True][0], got[False][0]):
        assert torch.equal(a, b)
    assert torch.equal(got[True][1], got[False][1])
    assert float(got[False][0][0].abs().sum()) > 0


def test_backbone_after_deferred_pass_keeps_the_pass(eight, synth):
    eng, clouds = eight
    eng.load_state_dict(synth.seeded_state_dict(0, cls_bias=-4.6))
    eng.set_head_defer(False)
    eng.infer_batch(clouds[:2])
    ref = [eng.fetch(0, "box").clone(), eng.fetch(1, "dir").clone()]
    eng.set_head_defer(True)
    eng.infer_batch(clouds[:2])
    vox, coors, npts, num = eng.voxelize(clouds[7])
    canvas = eng.scatter(eng.pfn(vox, coors, npts, num), coors, num)
    eng.backbone(canvas)  # overwrites the concat buffer and its statistics: the pass is materialised first
    assert torch.equal(eng.fetch(0, "box"), ref[0]) and torch.equal(eng.fetch(1, "dir"), ref[1])


def test_update_head_weights_after_deferred_pass_keeps_the_pass(eight, synth):
    eng, clouds = eight
    sd = synth.seeded_state_dict(0, cls_bias=-4.6)
    eng.load_state_dict(sd)
    eng.set_head_defer(False)
    eng.infer_batch(clouds[:2])
    ref = [eng.fetch(1, "box").clone(), eng.fetch(0, "dir").clone()]
    eng.set_head_defer(True)
    eng.infer_batch(clouds[:2])
    new = {k: (torch.as_tensor(sd[k]).to(eng.device).float() * 1.5 + 0.01).contiguous() for k in eng.HEAD_KEYS}
    eng.update_head_weights(new)
    assert torch.equal(eng.fetch(1, "box"), ref[0]) and torch.equal(eng.fetch(0, "dir"), ref[1])  # the logits of the weights the pass ran with
    eng.infer_batch(clouds[:2])
    assert not torch.equal(eng.fetch(1, "box"), ref[0])  # the next pass sees the new image
    d, f = both_modes(eng, clouds[:2], 0)
    assert_same(d, f, "after update_head_weights")


def test_nuscene_fp32(synth):
    eng = load_pkg("engine").Engine(make_cfg(synth, "nuscene"), max_batch=3)
    eng.load_state_dict(synth.seeded_state_dict(0, cls_bias=-3.0, num_anchor_per_loc=eng.num_anchor_per_loc))
    clouds = [torch.from_numpy(synth.lidar_cloud("nuscene", seed=1 + i)).cuda() for i in range(3)]
    for nms_mode in (0, 1):
        d, f = both_modes(eng, clouds, nms_mode)
        assert assert_same(d, f, f"nuscene nms {nms_mode}") > 0


@pytest.mark.parametrize("name,precision", [("nuscene_10class", "fp32"), ("nuscene", "fp16")])
def test_other_plans_keep_the_full_head(synth, monkeypatch, name, precision):
    eng_mod = load_pkg("engine")
    shape = "nuscene"
    clouds = [torch.from_numpy(synth.lidar_cloud(shape, seed=1 + i)).cuda() for i in range(2)]
    res = []
    for env_off in (False, True):
        if env_off:
            monkeypatch.setenv("PP_HEAD_DEFER", "0")
        eng = eng_mod.Engine(make_cfg(synth, name), max_batch=2, precision=precision)
        eng.load_state_dict(synth.seeded_state_dict(0, cls_bias=-3.0, num_anchor_per_loc=eng.num_anchor_per_loc))
        assert not eng.head_defer_active()
        det, cnt = eng.infer_batch(clouds)
        torch.cuda.synchronize()
        res.append((det.clone(), cnt.clone()))
        del eng
    assert_same(res[0], res[1], f"{name} {precision}")


def test_env_override_switches_a_capable_plan_off(synth, monkeypatch):
    monkeypatch.setenv("PP_HEAD_DEFER", "0")
    eng = load_pkg("engine").Engine(make_cfg(synth, "nuscene"), max_batch=1)
    eng.load_state_dict(synth.seeded_state_dict(0, cls_bias=-3.0))
    assert not eng.head_defer_active()
    eng.set_head_defer(True)
    assert not eng.head_defer_active()
