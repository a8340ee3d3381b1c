"""Post-processing at non-default NMS settings and on every selection path (-m gpu): the kernels of csrc/postprocess.hip
against the CPU oracle on the inputs of tests/postprocess_cases.py.  tests/test_postprocess_paths_cpu.py asserts, without a
GPU, that each case reaches the path it is named after; here the device has to give the oracle's answer on it: selection
exactly (anchor ids, their order, score bits, -1 padding), detections by count and within 2e-5 (the tolerance of
test_postprocess_stage_exact), AABB mode without any margin (iou_plus1 is the oracle's fp32 operation sequence), rotated mode
on seeds whose reference IoUs all stay 1e-4 away from the threshold."""
import numpy as np
import pytest
import torch

import postprocess_cases as P
from conftest import load_pkg
from oracle import c_oracle as C
from oracle import pp_oracle as O

pytestmark = pytest.mark.gpu


def _cfg(synth):
    cfg = P.small_config(synth)
    cfg["device"] = torch.device("cuda:0")
    return cfg


@pytest.fixture(scope="module")
def engine_of(synth):
    """One Engine per (nms_pre_max, nms_post_max, nms_iou_threshold, score_threshold), kept for the module."""
    eng_mod = load_pkg("engine")
    cache = {}

    def get(pre, post, iou, thr=0.05):
        key = (pre, post, iou, thr)
        if key not in cache:
            cache[key] = eng_mod.Engine(_cfg(synth), nms_pre_max=pre, nms_post_max=post, nms_iou_threshold=iou, score_threshold=thr)
            c = cache[key].cfg
            assert (c.nms_pre_max, c.nms_post_max) == (pre, post) and cache[key].A == P.A
        return cache[key]

    yield get
    cache.clear()


@pytest.fixture(scope="module")
def dev_r():
    """Recipe R on the device, per seed: (logits, box, dir, mask)."""
    cache = {}

    def get(seed):
        if seed not in cache:
            cache[seed] = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in P.recipe_r(seed))
        return cache[seed]

    return get


# ------------------------------------------------------------------ selection
@pytest.mark.parametrize("case", P.SELECT_CASES)
@pytest.mark.parametrize("K,thr", P.SELECT_PARAMS)
def test_select_candidates_equals_oracle(K, thr, case, engine_of, dev_r):
    ref = P.select_reference(case, K, thr)
    if ref is None:  # S4 exists only where the boundary logits are safe from the last bit of exp (see postprocess_cases.boundary_pair)
        assert case == "S4-boundary" and not P.s4_usable(thr) and thr != 0.05
        return
    logits, mask = P.select_inputs(case, K, thr)
    eng = engine_of(K, min(K, 300), 0.1, thr)
    _, box, dr, _ = dev_r(P.SELECT_SEED)
    idx, score, count = eng.select_candidates(torch.tensor(logits).cuda(), box, dr, torch.tensor(mask).cuda())
    idx, score, count = idx.cpu().numpy(), score.cpu().numpy(), count.cpu().numpy()
    assert idx.shape == score.shape == (3, K)
    want_idx = np.full((3, K), -1, np.int32)
    want_score = np.zeros((3, K), np.float32)
    for c, r in enumerate(ref):
        want_idx[c, :r["idx"].size] = r["idx"]
        want_score[c, :r["idx"].size] = r["score"]
    assert list(count) == [r["idx"].size for r in ref], (case, K, thr, list(count))
    for c in range(3):
        bad = np.nonzero(idx[c] != want_idx[c])[0]
        assert bad.size == 0, (case, K, thr, f"class {c}: first differing position {int(bad[0])}: anchor {int(idx[c, bad[0]])} "
                               f"score {float(score[c, bad[0]])!r}, oracle {int(want_idx[c, bad[0]])} {float(want_score[c, bad[0]])!r}")
    assert np.array_equal(score.view(np.uint32), want_score.view(np.uint32)), (case, K, thr)


# ------------------------------------------------------------------ NMS depth
@pytest.mark.parametrize("case", list(P.NMS_CASES))
def test_postprocess_equals_oracle(case, engine_of, dev_r):
    pre, post, iou, mode, seed = P.NMS_CASES[case]
    ref, counts, info, margin = P.nms_reference(case)
    eng = engine_of(pre, post, iou)
    logits, box, dr, mask = dev_r(seed)
    det, cnt = eng.postprocess(logits, box, dr, mask, nms_mode=1 if mode == "rotated" else 0)
    cnt = cnt.cpu().numpy()
    det = det[:int(cnt[0])].cpu().numpy()
    if list(cnt[1:4]) != counts:  # trace it: the selection first, then the first differing row
        idx = eng.select_candidates(logits, box, dr, mask)[0].cpu().numpy()
        sel_ok = [bool(np.array_equal(idx[c, :info[c]["idx"].size], info[c]["idx"])) for c in range(3)]
        off = np.concatenate([[0], np.cumsum(cnt[1:4])])
        first = []
        for c in range(3):
            got, want = det[off[c]:off[c + 1], 7], ref[sum(counts[:c]):sum(counts[:c + 1]), 7]
            n = min(got.size, want.size)
            d = np.nonzero(got[:n] != want[:n])[0]
            first.append(int(d[0]) if d.size else n)
        raise AssertionError((case, "counts", list(cnt[1:4]), "oracle", counts, "selection equal", sel_ok, "first differing row per class", first))
    assert int(cnt[0]) == sum(counts) == det.shape[0] > 0
    dev = float(np.abs(det - ref).max())
    print(f"[pp paths] {case}: {counts} rows, max |gpu - oracle| {dev:.2e}" + (f", reference IoU margin {margin:.2e}" if mode == "rotated" else ""))
    assert np.array_equal(det[:, 8], ref[:, 8])
    assert np.array_equal(det[:, 7].view(np.uint32), ref[:, 7].view(np.uint32))  # scores pass through as bits
    np.testing.assert_allclose(det, ref, rtol=0, atol=2e-5)


# ------------------------------------------------------------------ whole network, batched, K = 1153
CLS_BIAS = None
CLOUD_SEEDS = (1000, 1001, 1002)


def test_whole_network_batched_at_k1153(synth):
    """pp_infer_batch with nms_pre_max 1153 / nms_post_max 1024 / IoU 0.5 (cb = 19 column tiles: post_cand_b, nms_mask and
    nms_reduce index by a K that is no multiple of 64), three frames, AABB mode, head deferral on and off: each frame's
    detections are the parameterised oracle's on that frame's own logits (counts exactly, rows within 2e-5), and the two head
    modes are bit-equal.
    cls_bias None (the random-init head) was the first value tried and holds: candidates per class on an MI355X
    [40990, 2806, 7823] / [36503, 2346, 6684] / [36093, 2328, 6448] for the three frames (every class above 1153), rows
    [575, 687, 775] / [567, 655, 747] / [583, 666, 742], the sweeps ending at positions 1144 .. 1152 (tile 18, through the
    far-tile fold); largest deviation from the oracle 7.6e-6 on boxes up to 138 m."""
    eng = load_pkg("engine").Engine(_cfg(synth), max_batch=3, nms_pre_max=1153, nms_post_max=1024, nms_iou_threshold=0.5)
    eng.load_state_dict(synth.seeded_state_dict(0, cls_bias=CLS_BIAS))
    clouds = [torch.from_numpy(synth.lidar_cloud("eight_20cm", seed=s)).cuda() for s in CLOUD_SEEDS]
    g = P.geometry()
    out = {}
    for on in (True, False):
        eng.set_head_defer(on)
        assert eng.head_defer_active() == on
        det, cnt = eng.infer_batch(clouds, nms_mode=0)
        torch.cuda.synchronize()
        out[on] = (det.clone(), cnt.clone())
    assert torch.equal(out[True][1], out[False][1])
    assert torch.equal(out[True][0], out[False][0])
    det, cnt = out[False][0].cpu().numpy(), out[False][1].cpu().numpy()
    assert det.shape == (3, 3 * 1024, 9)
    for f in range(3):  # the last pass ran the full head: its tensors are the pass's own
        lg = {w: eng.fetch(f, w).cpu().numpy() for w in ("cls", "box", "dir", "mask")}
        ref, counts, info = O.postprocess(lg["cls"], lg["box"], lg["dir"], lg["mask"].astype(bool), g["anchors"], g["class_masks"], g["center_limit"],
                                          "aabb", detail=True, nms_fn=C.nms_aabb, pre_max=1153, post_max=1024, iou_thr=0.5)
        n = int(cnt[f, 0])
        dev = float(np.abs(det[f, :n] - ref).max()) if n == ref.shape[0] and n else float("nan")
        print(f"[pp paths] whole network frame {f}: candidates per class {[i['n_cand'] for i in info]}, rows {counts}, "
              f"max |gpu - oracle| {dev:.2e}, largest box field {float(np.abs(ref[:, :6]).max()) if ref.size else 0.0:.1f}")
        if f == 0:
            assert max(i["n_cand"] for i in info) > 1153, [i["n_cand"] for i in info]
        assert list(cnt[f, 1:4]) == counts and n == sum(counts)
        assert np.array_equal(det[f, :n, 8], ref[:, 8])
        np.testing.assert_allclose(det[f, :n], ref, rtol=0, atol=2e-5)


# ------------------------------------------------------------------ argument errors
@pytest.mark.parametrize("kw,field", [(dict(nms_pre_max=0), "nms_pre_max"), (dict(nms_pre_max=4097, nms_post_max=300), "nms_pre_max"),
                                      (dict(nms_pre_max=4096, nms_post_max=1025), "nms_post_max"),
                                      (dict(nms_pre_max=200, nms_post_max=201), "nms_post_max must not exceed nms_pre_max"),
                                      (dict(score_threshold=0.0), "score_threshold"), (dict(score_threshold=1.0), "score_threshold")])
def test_bad_nms_settings_are_rejected_by_pp_create(kw, field, synth):
    lib = load_pkg("_lib").load()
    with pytest.raises(RuntimeError, match="pp_create failed") as e:
        load_pkg("engine").Engine(_cfg(synth), **kw)
    assert field in str(e.value)
    assert field in lib.pp_last_error(None).decode()
