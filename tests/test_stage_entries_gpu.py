"""The single-stage entry points against the batched pass (-m gpu).  pp_voxelize, pp_anchor_mask, pp_pfn, pp_postprocess and
pp_select_candidates run the kernels of pp_infer_batch on ONE frame that is handed over by value (slot 0's scratch beside the
caller's tensors) instead of being looked up in the frame table by blockIdx.z.  Three distinct frames are the smallest case in
which a wrong frame lookup shows: with one frame, or with equal frames, it cannot.  Everything here is bit for bit; the same code
computes both sides."""
import numpy as np
import pytest
import torch

from conftest import load_pkg

pytestmark = pytest.mark.gpu

FULL, RAGGED, EMPTY = 0, 1, 2


@pytest.fixture(scope="module")
def setup(synth):
    """The config, weights and clouds of test_batched_frames_equal_single_frames; the full head in every pass, so that the box / dir
    tensors fetched after a pass are the ones its post-processing read."""
    cfg = synth.load_config("nuscene")
    cfg["device"] = torch.device("cuda:0")
    eng = load_pkg("engine").Engine(cfg, max_batch=3)
    eng.load_state_dict(synth.seeded_state_dict(2, cls_bias=-3.0))
    eng.set_head_defer(False)
    assert not eng.head_defer_active()
    clouds = [torch.from_numpy(synth.lidar_cloud("nuscene", seed=10)).cuda(),
              torch.from_numpy(synth.lidar_cloud("nuscene", seed=11, n_points=5000)).cuda(),
              torch.zeros((0, 4), dtype=torch.float32).cuda()]
    return eng, clouds


def _pass(eng, clouds, mode):
    det, cnt = eng.infer_batch(clouds, nms_mode=mode)
    torch.cuda.synchronize()
    return det.clone(), cnt.clone()


def _kept_rows_are_selected_in_order(eng, lg, det, cnt, sel):
    """Per class, every row pp_postprocess kept is an entry of pp_select_candidates' list -- same score bits, and the box the
    device decodes for that entry's anchor (pp_box_decode: the same device function) -- met in the list's order."""
    idx, score, count = (t.cpu().numpy() for t in sel)
    decode = load_pkg("framework.box_torch_ops").box_decode
    anchors = torch.from_numpy(eng.anchors_np).cuda()
    det, cnt = det.cpu().numpy(), cnt.cpu().numpy()
    off = 0
    for c in range(eng.cfg.num_classes):
        kept = det[off:off + cnt[1 + c]]
        off += cnt[1 + c]
        assert count[c] >= cnt[1 + c], (c, count[c], cnt[1 + c])
        assert (idx[c, count[c]:] == -1).all() and (idx[c, :count[c]] >= 0).all()
        if count[c] == 0:
            continue
        ids = torch.from_numpy(idx[c, :count[c]].astype(np.int64)).cuda()
        boxes = decode(lg["box"][ids], anchors[ids]).cpu().numpy()
        sbits, j = score[c, :count[c]].view(np.uint32), 0
        for r, row in enumerate(kept):
            assert row[8] == c
            while j < count[c] and not (sbits[j] == row[7:8].view(np.uint32)[0] and np.array_equal(boxes[j, :6].view(np.uint32), row[:6].view(np.uint32))):
                j += 1
            assert j < count[c], f"class {c}: kept row {r} (score {row[7]!r}) is not in the selection behind kept row {r - 1}"
            j += 1


def test_stage_entries_equal_the_batched_pass(setup):
    eng, clouds = setup
    first = {0: _pass(eng, clouds, 0)}
    assert int(first[0][1][FULL, 0]) > 0 and int(first[0][1][RAGGED, 0]) > 0 and int(first[0][1][EMPTY, 0]) == 0
    lg = [{w: eng.fetch(f, w) for w in ("cls", "box", "dir", "mask", "coors", "num", "feat")} for f in range(3)]
    nums = [int(l["num"][0]) for l in lg]
    assert nums[FULL] > nums[RAGGED] > 0 and nums[EMPTY] == 0  # three different frames

    # ---- the pillar stages.  They share slot 0's scratch with frame 0 of a pass and write only the caller's tensors.
    for f in (FULL, RAGGED):
        voxels, coors, npts, num = eng.voxelize(clouds[f])
        n = int(num[0])
        assert n == nums[f], (f, n, nums[f])
        assert torch.equal(coors[:n], lg[f]["coors"][:n]), f
        assert torch.equal(eng.anchor_mask(coors, num), lg[f]["mask"]), f
        assert torch.equal(eng.pfn(voxels, coors, npts, num)[:n], lg[f]["feat"][:n]), f
    _, coors, _, num = eng.voxelize(clouds[EMPTY])
    assert int(num[0]) == 0
    assert not eng.anchor_mask(coors, num).any() and not lg[EMPTY]["mask"].any()

    # ---- post-processing, both NMS modes: a batched pass per mode, the entry on the tensors that pass left
    for mode in (0, 1):
        if mode not in first:
            first[mode] = _pass(eng, clouds, mode)
            for f in range(3):  # the network does not depend on the mode
                assert all(torch.equal(eng.fetch(f, w), lg[f][w]) for w in ("cls", "box", "dir", "mask")), (mode, f)
        det_b, cnt_b = first[mode]
        for f in (FULL, RAGGED):
            det, cnt = eng.postprocess(lg[f]["cls"], lg[f]["box"], lg[f]["dir"], lg[f]["mask"], nms_mode=mode)
            assert torch.equal(cnt, cnt_b[f]), (mode, f, cnt.tolist(), cnt_b[f].tolist())
            assert torch.equal(det, det_b[f]), (mode, f)
            if mode == 0:  # pp_select_candidates prepares AABB boxes; its keys do not depend on the mode
                sel = eng.select_candidates(lg[f]["cls"], lg[f]["box"], lg[f]["dir"], lg[f]["mask"])
                _kept_rows_are_selected_in_order(eng, lg[f], det, cnt, sel)
    assert not torch.equal(first[0][0][FULL], first[0][0][RAGGED])

    # ---- the entries left the frame tables and slot 0 as a pass needs them
    for mode in (0, 1):
        det, cnt = _pass(eng, clouds, mode)
        assert torch.equal(cnt, first[mode][1]) and torch.equal(det, first[mode][0]), mode
