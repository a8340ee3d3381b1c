"""framework.gt_sampler: ground-truth database sampling for the training loader -- the `# sample` slot of the reference's
GenericDataset.__getitem__ (dataset.py:123), which the reference leaves empty.  A build-side extension in the style of SECOND /
PointPillars: recorded objects are pasted into a frame at their recorded pose until every class reaches its target count.

    db = build_database(config, ["infos_train.pkl"]); db.save(data_root / "gt_database.npz")
    config["gt_sampler"] = {"database": "gt_database.npz", "sample_groups": {"vehicle": 15, "pedestrian": 10}, "remove_points": True}

The database lives on the device; membership, ordered extraction, the greedy collision rejection and the paste run in
csrc/gt_sample.hip (Engine.gt_*).  The host keeps the bookkeeping of names / classes / difficulty and, in numpy mode, the draws."""
import numpy as np
import torch

from .. import _lib, kitti_io
from ..engine import engine_for

DB_KEYS = ("points", "offsets", "boxes", "names", "classes", "difficulty", "image_idx", "gt_idx", "class_off", "detect_class")


class GtDatabase:
    """Recorded objects, rows grouped by class in detect_class order (class c owns rows class_off[c] .. class_off[c+1]-1):
    points f32[T,4] object-local (xyz minus the box centre), offsets i64[n+1], boxes f32[n,7], names <U[n], classes i32[n] (1-based
    index into detect_class, as gt_classes), difficulty i32[n], image_idx i64[n], gt_idx i32[n] (row among the frame's detect-class
    annotations)."""

    def __init__(self, **kw):
        missing = [k for k in DB_KEYS if k not in kw]
        if missing:
            raise ValueError(f"GtDatabase: missing fields {missing}")
        self.points = np.ascontiguousarray(kw["points"], dtype=np.float32).reshape(-1, 4)
        self.offsets = np.ascontiguousarray(kw["offsets"], dtype=np.int64)
        self.boxes = np.ascontiguousarray(kw["boxes"], dtype=np.float32).reshape(-1, 7)
        self.names = np.asarray(kw["names"]).astype(str)
        self.classes = np.ascontiguousarray(kw["classes"], dtype=np.int32)
        self.difficulty = np.ascontiguousarray(kw["difficulty"], dtype=np.int32)
        self.image_idx = np.ascontiguousarray(kw["image_idx"], dtype=np.int64)
        self.gt_idx = np.ascontiguousarray(kw["gt_idx"], dtype=np.int32)
        self.class_off = np.ascontiguousarray(kw["class_off"], dtype=np.int64)
        self.detect_class = [str(c) for c in kw["detect_class"]]
        n = self.boxes.shape[0]
        if (self.offsets.shape != (n + 1,) or self.offsets[0] != 0 or (np.diff(self.offsets) < 0).any() or self.offsets[-1] != self.points.shape[0]
                or any(a.shape[0] != n for a in (self.names, self.classes, self.difficulty, self.image_idx, self.gt_idx))
                or self.class_off.shape != (len(self.detect_class) + 1,) or self.class_off[0] != 0 or self.class_off[-1] != n
                or (np.diff(self.class_off) < 0).any()):
            raise ValueError("GtDatabase: inconsistent fields")
        for c in range(len(self.detect_class)):
            if (self.classes[self.class_off[c]:self.class_off[c + 1]] != c + 1).any():
                raise ValueError("GtDatabase: rows are not grouped by class in detect_class order")
        self._dev = {}

    def __len__(self):
        return int(self.boxes.shape[0])

    def save(self, path):
        """One .npz of plain arrays (no pickled objects)."""
        np.savez_compressed(path, points=self.points, offsets=self.offsets, boxes=self.boxes, names=self.names.astype("<U32"),
                            classes=self.classes, difficulty=self.difficulty, image_idx=self.image_idx, gt_idx=self.gt_idx,
                            class_off=self.class_off, detect_class=np.array(self.detect_class, dtype="<U32"))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(**{k: z[k] for k in DB_KEYS})

    def device(self, eng):
        """(points f32[T,4], offsets i64[n+1], boxes f32[n,7]) on the engine's device, uploaded once."""
        key = str(eng.device)
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(a).to(eng.device) for a in (self.points, self.offsets, self.boxes))
        return self._dev[key]


def build_database(config, info_paths, min_points=5):
    """Load and remap the infos as GenericDataset does; per frame upload the cloud, take the annotations whose name is in
    detect_class, count and extract their points on the device, and keep the objects with at least min_points points.  difficulty is
    the info's own where it has one, else create_info's count (boxes grown by (1.2, 0.5, 8)).  One host sync per frame (the total)."""
    from pathlib import Path
    root = Path(config["data_root"])
    detect_class = list(config["detect_class"])
    infos = kitti_io.load_infos(root, info_paths)
    kitti_io.remap_classes(infos)
    eng = engine_for(config)
    rec = []  # per object: (class, frame order, gt_idx, ...)
    for fi, info in enumerate(infos):
        annos = info["annos"]
        names = np.asarray(annos["name"]).astype(str)
        m = np.array([n in detect_class for n in names], dtype=np.bool_)
        if not m.any():
            continue
        boxes = np.concatenate([annos["location"][m], annos["dimensions"][m], annos["rotation_y"][m][..., np.newaxis]], axis=1).astype(np.float32)
        pts = kitti_io.read_velodyne(root / info["velodyne_path"], config["num_point_features"])
        pts_d = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).to(eng.device)
        box_d = torch.from_numpy(boxes).to(eng.device)
        off_p, off_b = [0, pts.shape[0]], [0, boxes.shape[0]]
        counts = eng.gt_count(pts_d, off_p, box_d, off_b)
        obj_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=eng.device), torch.cumsum(counts.to(torch.int64), 0)])
        if "difficulty" in annos:
            diff = np.asarray(annos["difficulty"])[m].astype(np.int32)
            oh = obj_off.cpu().numpy()
        else:
            dcount = eng.gt_count(pts_d, off_p, box_d, off_b, kitti_io.DIFFICULTY_EXTRA)
            host = torch.cat([obj_off, dcount.to(torch.int64)]).cpu().numpy()
            oh, diff = host[:boxes.shape[0] + 1], host[boxes.shape[0] + 1:].astype(np.int32)
        local = eng.gt_extract(pts_d, off_p, box_d, off_b, obj_off, int(oh[-1])).cpu().numpy()
        fn = names[m]
        for j in range(boxes.shape[0]):
            if oh[j + 1] - oh[j] >= min_points:
                rec.append((detect_class.index(fn[j]), fi, j, local[oh[j]:oh[j + 1]], boxes[j], fn[j], int(diff[j]), int(info.get("image_idx", fi))))
    rec.sort(key=lambda r: (r[0], r[1], r[2]))  # grouped by class, then frame and annotation order
    n = len(rec)
    sizes = np.array([r[3].shape[0] for r in rec], dtype=np.int64)
    cls0 = np.array([r[0] for r in rec], dtype=np.int64)
    return GtDatabase(points=np.concatenate([r[3] for r in rec]) if n else np.zeros((0, 4), np.float32),
                      offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                      boxes=np.stack([r[4] for r in rec]) if n else np.zeros((0, 7), np.float32),
                      names=np.array([r[5] for r in rec], dtype="<U32"), classes=(cls0 + 1).astype(np.int32),
                      difficulty=np.array([r[6] for r in rec], dtype=np.int32), image_idx=np.array([r[7] for r in rec], dtype=np.int64),
                      gt_idx=np.array([r[2] for r in rec], dtype=np.int32),
                      class_off=np.concatenate([[0], np.cumsum(np.bincount(cls0, minlength=len(detect_class)))]).astype(np.int64),
                      detect_class=detect_class)


class GtSampler:
    """Host side of the sampling step: how many objects of each class a frame asks for, which ones (numpy mode), and the cut at
    PP_AUG_MAX_BOXES.  config["gt_sampler"] = {"database": path under data_root, "sample_groups": {class: target count},
    "remove_points": bool}.  Raises ValueError (before anything is launched) for a class in sample_groups that is not in
    detect_class, a negative target, and a database built for other classes."""

    def __init__(self, config, database):
        cfg = config["gt_sampler"]
        self.detect_class = list(config["detect_class"])
        groups = dict(cfg.get("sample_groups", {}))
        unknown = [c for c in groups if c not in self.detect_class]
        if unknown:
            raise ValueError(f"gt_sampler: sample_groups names {unknown}, which detect_class {self.detect_class} does not hold")
        if any(int(v) < 0 for v in groups.values()):
            raise ValueError("gt_sampler: a negative target count")
        if list(database.detect_class) != self.detect_class:
            raise ValueError(f"gt_sampler: the database was built for {database.detect_class}, the config detects {self.detect_class}")
        self.db = database
        self.targets = np.array([int(groups.get(c, 0)) for c in self.detect_class], dtype=np.int64)
        self.remove_points = bool(cfg.get("remove_points", True))
        self.n_per_class = np.diff(database.class_off).astype(np.int64)

    def counts(self, gt_classes):
        """k_c = min(max(target_c - existing boxes of class c, 0), n_c) for the frame's 1-based gt_classes: i64[C]."""
        have = np.bincount(np.asarray(gt_classes, dtype=np.int64), minlength=len(self.detect_class) + 1)[1:len(self.detect_class) + 1]
        return np.minimum(np.maximum(self.targets - have, 0), self.n_per_class)

    @staticmethod
    def cut(k, n_existing):
        """The candidate list (class order, then draw order) cut so that existing + candidates <= PP_AUG_MAX_BOXES: the counts kept."""
        room = max(_lib.PP_AUG_MAX_BOXES - int(n_existing), 0)
        out = np.zeros_like(k)
        for c in range(len(k)):
            out[c] = min(int(k[c]), room)
            room -= int(out[c])
        return out

    def draw_numpy(self, gt_classes):
        """numpy mode: database rows of the frame's candidates.  np.random.choice(n_c, k_c, replace=False) per class in detect_class
        order whenever k_c > 0 (no draw otherwise), each before the cut; these draws come in front of the frame's draw_frame draws."""
        k = self.counts(gt_classes)
        kept = self.cut(k, len(gt_classes))
        rows = []
        for c in range(len(k)):
            if k[c] > 0:
                pick = np.random.choice(int(self.n_per_class[c]), int(k[c]), replace=False)
                rows.append(self.db.class_off[c] + pick[:kept[c]])
        return np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)


def paste_frames(eng, sampler, clouds, gts, cand_rows=None, draw=None):
    """The device part for nb frames: select -> paste.  clouds: nb host f32[n,4] arrays; gts: the frames' class-filtered ground truth
    (dicts of names, classes, boxes, difficulty, valid); candidates either as host database rows per frame (cand_rows, numpy mode) or
    drawn on the device (draw = (seed, epoch, sample indices), device mode).  Returns per frame (points f32[n',4] device tensor, the
    ground truth with the accepted objects appended -- valid True --, a record for the tests).  Cost beyond the launches: one small
    D2H (accept flags, the candidate rows and the output sizes), which the output allocation waits for."""
    db = sampler.db
    nb = len(clouds)
    dev = eng.device
    dbp, dbo, dbb = db.device(eng)
    pt_off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int64).tolist()
    box_off = np.concatenate([[0], np.cumsum([g["boxes"].shape[0] for g in gts])]).astype(np.int64).tolist()
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(clouds), dtype=np.float32).reshape(-1, 4)).to(dev)
    boxes = torch.from_numpy(np.concatenate([g["boxes"] for g in gts]).reshape(-1, 7).astype(np.float32)).to(dev)
    if draw is not None:
        k = np.stack([sampler.cut(sampler.counts(g["classes"]), len(g["classes"])) for g in gts])
        cand_idx, cand_off = eng.gt_draw(draw[0], draw[1], draw[2], db.class_off.tolist(), k)
    else:
        rows = np.concatenate(cand_rows) if nb else np.zeros(0, np.int64)
        if rows.size and (rows.min() < 0 or rows.max() >= len(db)):
            raise ValueError("gt_sampler: a candidate row outside the database")
        cand_off = np.concatenate([[0], np.cumsum([len(r) for r in cand_rows])]).astype(np.int64).tolist()
        cand_idx = torch.from_numpy(rows.astype(np.int32)).to(dev)
    cand = dbb[cand_idx.long()] if cand_off[-1] else torch.zeros((0, 7), dtype=torch.float32, device=dev)
    accept = eng.gt_select(boxes, box_off, cand, cand_off)
    out_n, blk = eng.gt_paste_count(pts, pt_off, cand, cand_idx, accept, cand_off, dbp, dbo, sampler.remove_points)
    host = torch.cat([out_n, accept.to(torch.int32), cand_idx]).cpu().numpy()  # the one D2H
    Gc = cand_off[-1]
    n_h, acc_h, idx_h = host[:nb], host[nb:nb + Gc].astype(bool), host[nb + Gc:].astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum(n_h)]).astype(np.int64).tolist()
    out = eng.gt_paste(pts, pt_off, cand, cand_idx, accept, cand_off, dbp, dbo, blk, out_off, sampler.remove_points)
    res = []
    for f in range(nb):
        g, rows, acc = gts[f], idx_h[cand_off[f]:cand_off[f + 1]], acc_h[cand_off[f]:cand_off[f + 1]]
        take = rows[acc]
        new = dict(names=np.concatenate([g["names"], db.names[take]]),  # the wider of the two string types
                   classes=np.concatenate([g["classes"], db.classes[take]]).astype(np.int32),
                   boxes=np.concatenate([g["boxes"].reshape(-1, 7), db.boxes[take]]).astype(np.float32),
                   difficulty=np.concatenate([np.asarray(g["difficulty"]), db.difficulty[take].astype(np.asarray(g["difficulty"]).dtype)]),
                   valid=np.concatenate([g["valid"], np.ones(take.shape[0], np.bool_)]))
        record = dict(boxes=g["boxes"].reshape(-1, 7).copy(), cand_rows=rows.copy(), accept=acc.copy(), n_scene=int(clouds[f].shape[0]),
                      n_objects=int((db.offsets[take + 1] - db.offsets[take]).sum()))
        res.append((out[out_off[f]:out_off[f + 1]], new, record))
    return res
