"""CPU: ground-truth database sampling without a device.  The numpy restatement (tests/gtsample_ref.py) is held to the reference's
tables, counts, collision matrix and removal (tests/golden/gtsample_small.npz); the sampler's host logic (k_c, the cut at
PP_AUG_MAX_BOXES, the config errors, the numpy-mode stream consumption) to the restatement and to np.random calls made by hand; the
database file round-trips; and a dataset without the config key never enters the sampler."""
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden, load_pkg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gtsample_ref as S  # noqa: E402

G = golden("gtsample_small")
NEW = {"pp_gt_count": 9, "pp_gt_extract": 10, "pp_gt_select": 8, "pp_gt_paste_count": 15, "pp_gt_paste": 17, "pp_gt_draw": 11}
CLASSES = ["vehicle", "pedestrian", "cyclist"]


def test_symbols_declared_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pp_hip.h")).read(), flags=re.S)
    lib = load_pkg("_lib")
    for name, nargs in NEW.items():
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr)
        assert m, f"include/pp_hip.h does not declare {name}"
        assert len(m.group(1).split(",")) == nargs
        assert name in lib.PROTOTYPES and len(lib.PROTOTYPES[name][1]) == nargs, name
    assert lib.PP_GT_CHUNK == int(re.search(r"#define PP_GT_CHUNK (\d+)", hdr).group(1))
    assert S.MAX_BOXES == lib.PP_AUG_MAX_BOXES


def test_ref_membership_and_counts_against_golden():
    for f in range(3):
        pts, boxes = G[f"points_{f}"], G[f"boxes_{f}"]
        assert np.array_equal(S.member_table(pts, boxes), G[f"table_{f}"])
        assert np.array_equal(S.count(pts, boxes), G[f"num_points_{f}"])
        assert np.array_equal(S.count(pts, boxes, G["extra"]), G[f"difficulty_{f}"])
    assert tuple(np.float32(G["extra"])) == tuple(np.float32(S.DIFFICULTY_EXTRA))
    local, off = S.extract(G["points_0"], G["boxes_0"])
    assert np.array_equal(np.diff(off), G["num_points_0"]) and local.shape == (off[-1], 4)
    j = 4  # order and centring of one object
    want = G["points_0"][G["table_0"][:, j]]
    assert np.array_equal(local[off[j]:off[j + 1], 3], want[:, 3])
    assert np.array_equal(local[off[j]:off[j + 1], :3], want[:, :3] - G["boxes_0"][j, :3])


def test_ref_select_against_golden():
    ex, cand = G["sel_existing"], G["sel_cand"]
    allb = np.concatenate([ex, cand])
    mine = S.collision_matrix(cand, allb)
    off = ~np.eye(len(cand), len(allb), len(ex), dtype=bool)
    assert np.array_equal(mine[off], G["sel_collision"][off])
    assert np.array_equal(S.select(ex, cand), G["sel_accept"])
    assert G["sel_accept"].tolist() == [False, True, False, True, True]  # invalid-box hit, free, hit by accepted, hit by rejected only
    # a rejected candidate blocks nobody, an accepted one does
    assert S.select(ex, cand[[1, 2, 3]]).tolist() == [True, False, True] and S.select(ex, cand[[2, 3]]).tolist() == [True, False]
    assert S.select(np.zeros((0, 7)), cand[:1]).tolist() == [True] and S.select(ex, np.zeros((0, 7))).tolist() == []


def test_ref_paste_against_golden():
    pts, rm = G["points_0"], G["boxes_0"][G["remove_boxes"]]
    db_points = np.arange(40, dtype=np.float32).reshape(10, 4)
    db_off = np.array([0, 3, 4, 10])
    out = S.paste(pts, rm, [2, 1, 0], [True, True, True], db_points, db_off)
    n_obj = 6 + 1 + 3
    assert np.array_equal(out[n_obj:], G["remove_points"])
    assert np.array_equal(out[:6, :3], db_points[4:10, :3] + rm[0, :3]) and np.array_equal(out[6:7, 3], db_points[3:4, 3])
    assert np.array_equal(S.paste(pts, rm, [2, 1, 0], [False] * 3, db_points, db_off), pts)
    assert S.paste(pts, rm, [2, 1, 0], [True] * 3, db_points, db_off, remove=False).shape[0] == n_obj + pts.shape[0]
    # an index outside the database counts as not accepted
    assert np.array_equal(S.paste(pts, rm[:1], [3], [True], db_points, db_off), pts)


def _database(n=(6, 3, 0)):
    gts = load_pkg("framework.gt_sampler")
    tot = sum(n)
    rng = np.random.default_rng(3)
    sizes = rng.integers(5, 9, tot)
    cls = np.concatenate([np.full(k, c + 1) for c, k in enumerate(n)]).astype(np.int32)
    return gts.GtDatabase(points=rng.normal(size=(int(sizes.sum()), 4)).astype(np.float32), offsets=np.concatenate([[0], np.cumsum(sizes)]),
                          boxes=rng.normal(size=(tot, 7)).astype(np.float32), names=np.array([CLASSES[c - 1] for c in cls]), classes=cls,
                          difficulty=np.arange(tot, dtype=np.int32), image_idx=np.arange(tot) // 2, gt_idx=np.arange(tot, dtype=np.int32) % 2,
                          class_off=np.concatenate([[0], np.cumsum(n)]), detect_class=CLASSES)


def _config(groups, **kw):
    return dict(detect_class=list(CLASSES), gt_sampler=dict(database="db.npz", sample_groups=groups, **kw))


def test_database_round_trip(tmp_path):
    gts = load_pkg("framework.gt_sampler")
    db = _database()
    db.save(tmp_path / "db.npz")
    with np.load(tmp_path / "db.npz", allow_pickle=False) as z:  # data only
        assert {"points", "offsets", "boxes", "names", "classes", "difficulty", "image_idx", "gt_idx", "class_off"} <= set(z.files)
    back = gts.GtDatabase.load(tmp_path / "db.npz")
    for k in ("points", "offsets", "boxes", "classes", "difficulty", "image_idx", "gt_idx", "class_off"):
        assert np.array_equal(getattr(back, k), getattr(db, k)) and getattr(back, k).dtype == getattr(db, k).dtype, k
    assert back.names.tolist() == db.names.tolist() and back.detect_class == CLASSES and len(back) == 9
    with pytest.raises(ValueError):
        gts.GtDatabase(**{**{k: getattr(db, k) for k in gts.DB_KEYS}, "class_off": np.array([0, 5, 9, 9])})  # not grouped by class


def test_counts_cut_and_errors():
    gts = load_pkg("framework.gt_sampler")
    db = _database()
    s = gts.GtSampler(_config({"vehicle": 4, "pedestrian": 10}), db)
    assert s.remove_points and s.targets.tolist() == [4, 10, 0]
    for classes in ([], [1], [1, 1, 1, 1, 1, 2], [2, 3, 3], [1, 2] * 6):
        want = S.k_counts([4, 10, 0], classes, [6, 3, 0])
        assert np.array_equal(s.counts(np.array(classes, np.int32)), want), classes
    assert s.counts(np.array([], np.int32)).tolist() == [4, 3, 0] and s.counts(np.array([1] * 5, np.int32)).tolist() == [0, 3, 0]
    cap = load_pkg("_lib").PP_AUG_MAX_BOXES
    for k, n in (([4, 3, 0], 0), ([4, 3, 0], cap - 5), ([4, 3, 0], cap - 4), ([4, 3, 0], cap), ([4, 3, 0], cap + 3), ([0, 3, 2], cap - 4)):
        got = gts.GtSampler.cut(np.array(k), n)
        assert np.array_equal(got, S.cut(k, n)) and n + got.sum() <= max(cap, n), (k, n)
    assert gts.GtSampler.cut(np.array([4, 3, 0]), cap - 5).tolist() == [4, 1, 0]
    assert not gts.GtSampler(_config({}, remove_points=False), db).remove_points
    with pytest.raises(ValueError):
        gts.GtSampler(_config({"tram": 3}), db)  # unknown class
    with pytest.raises(ValueError):
        gts.GtSampler(_config({"vehicle": -1}), db)
    with pytest.raises(ValueError):
        gts.GtSampler(dict(_config({"vehicle": 3}), detect_class=["vehicle", "pedestrian"]), db)  # database built for other classes


def test_numpy_mode_stream_consumption():
    gts = load_pkg("framework.gt_sampler")
    db = _database()
    s = gts.GtSampler(_config({"vehicle": 4, "pedestrian": 3}), db)
    classes = np.array([1, 2], np.int32)  # k = (3, 2, 0)
    np.random.seed(12)
    rows = s.draw_numpy(classes)
    state = np.random.get_state()[1].copy(), np.random.get_state()[2]
    np.random.seed(12)
    a = np.random.choice(6, 3, replace=False)
    b = np.random.choice(3, 2, replace=False)
    assert np.array_equal(rows, np.concatenate([a, 6 + b]))
    assert np.array_equal(np.random.get_state()[1], state[0]) and np.random.get_state()[2] == state[1]
    np.random.seed(12)
    assert np.array_equal(S.draw_numpy([4, 3, 0], classes, db.class_off), rows)
    assert len(set(rows.tolist())) == len(rows) and (db.classes[rows] == [1, 1, 1, 2, 2]).all()
    # every k_c = 0: no draw is consumed
    np.random.seed(13)
    before = np.random.get_state()[1].copy(), np.random.get_state()[2]
    assert s.draw_numpy(np.array([1, 1, 1, 1] + [2] * 10, np.int32)).size == 0
    assert np.array_equal(np.random.get_state()[1], before[0]) and np.random.get_state()[2] == before[1]
    # the draws are made for the uncut k_c; the cut takes the front of the list
    cap = load_pkg("_lib").PP_AUG_MAX_BOXES
    many = np.array([3] * (cap - 4), np.int32)  # k = (4, 3, 0), room for 4
    np.random.seed(14)
    rows = s.draw_numpy(many)
    np.random.seed(14)
    a = np.random.choice(6, 4, replace=False)
    b = np.random.choice(3, 3, replace=False)
    nxt = np.random.random()
    assert np.array_equal(rows, a)
    np.random.seed(14)
    s.draw_numpy(many)
    assert np.random.random() == nxt


class _NoGtEngine:
    """Stands in for the engine of a dataset: any Engine.gt_* call is an error, the voxeliser returns one empty pillar."""
    device = torch.device("cpu")

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} was called")

    def voxelize(self, pts):
        z = torch.zeros
        return z((1, 4, 4)), z((1, 3), dtype=torch.int32), z(1, dtype=torch.int32), torch.ones(1, dtype=torch.int32)


class _Assigner:
    def create_mask_device(self, coors, num):
        return torch.ones(4, dtype=torch.uint8)

    def assign_batch(self, gl, masks):
        nb = len(gl)
        return torch.zeros((nb, 4), dtype=torch.int32), torch.zeros((nb, 4, 7)), torch.zeros((nb, 4)), torch.zeros((nb, 4), dtype=torch.int32)


def test_without_the_key_the_sampler_is_never_entered(tmp_path, monkeypatch):
    dsm = load_pkg("framework.dataset")
    gts = load_pkg("framework.gt_sampler")
    agm = load_pkg("framework.augmentation")
    boxes = G["boxes_0"][:3]
    G["points_2"].astype(np.float32).tofile(tmp_path / "000000.bin")
    info = {"velodyne_path": "000000.bin", "image_idx": 0, "img_shape": np.array([375, 1242], np.int32), "calib/R0_rect": np.eye(4),
            "calib/Tr_velo_to_cam": np.eye(4), "calib/P2": np.eye(4),
            "annos": {"name": np.array(["car", "person", "car"], dtype="<U10"), "location": boxes[:, :3].copy(), "dimensions": boxes[:, 3:6].copy(),
                      "rotation_y": boxes[:, 6].copy(), "num_points": np.full(3, 10, np.int32), "difficulty": np.zeros(3, np.int32)}}
    with open(tmp_path / "infos.pkl", "wb") as fh:
        pickle.dump([info], fh)
    cfg = dict(data_root=str(tmp_path), num_point_features=4, detect_class=list(CLASSES), detection_range=[-80, -80, -3, 80, 80, 1],
               grid_size=[8, 8, 1])

    def refuse(*a, **k):
        raise AssertionError("the sampler was entered")

    monkeypatch.setattr(gts, "paste_frames", refuse)
    monkeypatch.setattr(gts.GtSampler, "__init__", refuse)
    monkeypatch.setattr(gts.GtDatabase, "load", classmethod(refuse))
    eng = _NoGtEngine()
    monkeypatch.setattr(dsm.GenericDataset, "_engine", lambda self: eng)

    def run_frames(eng_, pts, pt_off, bx, cls, valid, box_off, draws, bv_range):
        g = bx.shape[0]
        return pts, bx, cls, torch.ones(g, dtype=torch.uint8), torch.tensor([g], dtype=torch.int32), None

    monkeypatch.setattr(agm, "run_frames", run_frames)
    ds = dsm.GenericDataset(cfg, ["infos.pkl"], object(), _Assigner())
    assert ds.sampler is None
    np.random.seed(4)
    ex = ds[0]
    nxt = np.random.random()
    np.random.seed(4)
    agm.draw_frame(G["points_2"].shape[0], 3, True, True)  # the frame's stream is the chain's draws alone
    assert np.random.random() == nxt
    assert ex["annos"]["gt_boxes"].shape == (3, 7) and ex["points"].shape == G["points_2"].shape
    with pytest.raises(ValueError):
        ds.export_samples([0])
    # with the key, the constructor is where the sampler starts (refused here); not for evaluation or augm=False
    cfg["gt_sampler"] = {"database": "db.npz", "sample_groups": {"vehicle": 2}}
    with pytest.raises(AssertionError):
        dsm.GenericDataset(cfg, ["infos.pkl"], object(), _Assigner())
    assert dsm.GenericDataset(cfg, ["infos.pkl"], object(), _Assigner(), augm=False).sampler is None
    assert dsm.GenericDataset(cfg, ["infos.pkl"], object(), _Assigner(), training=False).sampler is None
