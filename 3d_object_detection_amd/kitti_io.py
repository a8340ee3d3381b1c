"""Data formats either side of the hot path: the reference's evaluation loop reads KITTI-style
`velodyne/*.bin` clouds listed in `data_info.pkl` info files and writes the detections as one pickle
(`train.py:204-222`, `:258-265`; infos are produced by `create_info.py:33-113`).

  read_velodyne(path)            f32[N,4] cloud                                   (train.py:221-222)
  load_infos(root, info_paths)   concatenated info dicts                          (train.py:208-214)
  remap_classes(infos)           the reference's label clean-up, in place         (train.py:164-184)
  annos_from_records(...)        device detection records -> KITTI-style annos    (inference.py:124-138,724-737)
  run_sequence(...)              clouds -> annos through pp_infer_batch, B frames per pass, one D2H per pass
  save_detections / load_detections   the `dt_info` pickle                        (train.py:264-265)
  gt_from_annos(annos, ...)      annos -> (gt_classes, gt_boxes) as GenericDataset builds them (dataset.py:108-140, no augmentation)
  point_counts(points, boxes)    (num_points, difficulty) of an info's annotations   (create_info.py:159-183)
  sequence_loss(...)             validation loss and Metric over a labelled sequence: pp_infer_batch + pp_batch_loss per pass
  pointcloud2_to_points(msg)     sensor_msgs/PointCloud2 payload -> f32[N,4] on the device   (ros_node.py:55-59)

Host-side glue only: the compute stays in libpp_hip.so (engine.Engine).
"""
import os
import pickle

import numpy as np
import torch

from .engine import engine_for
from .framework.inference import get_start_result_anno

# train.py:171-184: dataset labels -> the three detection classes
CLASS_REMAP = {"car": "vehicle", "truck": "vehicle", "bus": "vehicle", "person": "pedestrian",
               "bicycle": "cyclist", "motorbike": "cyclist"}


def read_velodyne(path, num_features=4):
    """`np.fromfile(v_path, dtype=np.float32).reshape([-1, 4])` (train.py:222); a truncated file is an error here
    instead of a silent reshape failure."""
    raw = np.fromfile(os.fspath(path), dtype=np.float32)
    if raw.size % num_features:
        raise ValueError(f"{path}: {raw.size} floats is not a whole number of {num_features}-feature points")
    return raw.reshape(-1, num_features)


def load_infos(data_root, info_paths):
    """Concatenate the pickled info lists (train.py:208-214). Each info carries at least `velodyne_path` and,
    for evaluation, `annos` (name, location, dimensions, rotation_y, num_points, ...)."""
    infos = []
    for rel in info_paths:
        with open(os.path.join(os.fspath(data_root), rel), "rb") as f:
            infos += pickle.load(f)
    return infos


def remap_classes(infos):
    """In-place label clean-up of train.py:164-184: drop boxes without points, then map the dataset's labels onto
    vehicle / pedestrian / cyclist. Returns the number of 'person' boxes seen (the reference counts them)."""
    persons = 0
    for info in infos:
        annos = info.get("annos")
        if annos is None or len(annos["name"]) == 0:
            continue
        keep = np.asarray(annos["num_points"]) > 0
        for key in annos:
            annos[key] = annos[key][keep]
        names = annos["name"]
        persons += int((names == "person").sum())
        out = names.astype(object)
        for src, dst in CLASS_REMAP.items():
            out[names == src] = dst
        # a '<U7' source array would truncate 'pedestrian': widen like the reference's in-place writes cannot
        annos["name"] = out.astype("<U10")
    return persons


def annos_from_records(det, cnt, class_names):
    """det f32[nb,rows,9] (x,y,z,l,w,h,r,score,class), cnt i32[nb,1+C] on the HOST -> list of nb annos in the
    reference's result layout (inference.py:124-138 on top of get_start_result_anno :724-737)."""
    out = []
    for b in range(det.shape[0]):
        k = int(cnt[b, 0])
        anno = get_start_result_anno()
        if k > 0:
            rows = det[b, :k]
            anno["name"] = np.array([class_names[int(c)] for c in rows[:, 8]], dtype="<U10")
            anno["location"] = rows[:, :3].copy()
            anno["dimensions"] = rows[:, 3:6].copy()
            anno["rotation_y"] = rows[:, 6].copy()
            anno["score"] = rows[:, 7].copy()
        out.append(anno)
    return out


def run_sequence(config, clouds, class_names, batch=16, nms_mode=0):
    """The body of the reference's `infer()` loop (train.py:218-242) for a list of clouds (numpy f32[N,4] or paths
    of .bin files): frames go through pp_infer_batch `batch` at a time, one pinned D2H of the fixed-size records
    per pass. Returns the annos in frame order. The engine must hold committed weights (PointPillars.load_state_dict
    or Engine.load_state_dict)."""
    eng = engine_for(config)
    batch = max(1, min(int(batch), eng.max_batch))
    rows = eng.cfg.num_classes * eng.cfg.nms_post_max
    det_h = torch.zeros((batch, rows, 9), dtype=torch.float32).pin_memory()
    cnt_h = torch.zeros((batch, det_count_stride()), dtype=torch.int32).pin_memory()
    annos = []
    for i0 in range(0, len(clouds), batch):
        group = []
        for c in clouds[i0:i0 + batch]:
            pts = read_velodyne(c) if isinstance(c, (str, os.PathLike)) else np.ascontiguousarray(c, dtype=np.float32)
            group.append(torch.from_numpy(pts).to(eng.device, non_blocking=True))
        det, cnt = eng.infer_batch(group, nms_mode=nms_mode)
        nb = len(group)
        det_h[:nb].copy_(det, non_blocking=True)
        cnt_h[:nb].copy_(cnt, non_blocking=True)
        torch.cuda.current_stream(eng.device).synchronize()
        annos += annos_from_records(det_h[:nb].numpy(), cnt_h[:nb].numpy(), class_names)
    return annos


def det_count_stride():
    from . import _lib
    return 1 + _lib.PP_MAX_CLASSES


def save_detections(path, dt_annos):
    """`pickle.dump(dt_annos, f)` into <data_root>/<result_path>/<experiment>/<dt_info> (train.py:258-265)."""
    d = os.path.dirname(os.fspath(path))
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as f:
        pickle.dump(dt_annos, f)


def load_detections(path):
    with open(path, "rb") as f:
        return pickle.load(f)


# sensor_msgs/PointField datatype codes
_PC2_SIZES = {1: 1, 2: 1, 3: 2, 4: 2, 5: 4, 6: 4, 7: 4, 8: 8}


def pointcloud2_to_points(msg, device=None):
    """`np.asarray(list(pc2.read_points(msg)))[:, :4].astype(np.float32)` of the reference's ROS callback
    (ros_node.py:55-59) as one H2D copy of the raw payload + one unpack kernel: the first four fields of the message
    (in the message's field order, whatever their types, offsets and padding) become f32[N,4] on the device.
    `msg` is any object with the PointCloud2 attributes (data, fields[name/offset/datatype/count], point_step, row_step,
    width, height, is_bigendian); rospy itself is not needed."""
    import ctypes
    from . import _lib
    fields = sorted(msg.fields, key=lambda f: f.offset)  # read_points orders the struct by offset
    if len(fields) < 4:
        raise ValueError("PointCloud2 message has fewer than 4 fields")
    first = fields[:4]
    for f in first:
        if getattr(f, "count", 1) != 1:
            raise ValueError(f"field {f.name}: count != 1 is not supported")
        if f.datatype not in _PC2_SIZES:
            raise ValueError(f"field {f.name}: unknown datatype {f.datatype}")
    n = int(msg.width) * int(msg.height)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    raw = np.frombuffer(bytes(msg.data), dtype=np.uint8)
    need = (int(msg.height) - 1) * int(msg.row_step) + int(msg.width) * int(msg.point_step)
    if raw.size < need:
        raise ValueError(f"PointCloud2 data holds {raw.size} bytes, {need} needed")
    buf = torch.from_numpy(raw.copy()).to(dev, non_blocking=True)
    offs = (ctypes.c_int32 * 4)(*[int(f.offset) for f in first])
    dts = (ctypes.c_int32 * 4)(*[int(f.datatype) for f in first])
    with torch.cuda.device(dev):
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.load().pp_unpack_points(buf.data_ptr(), n, int(msg.width), int(msg.row_step), int(msg.point_step), offs, dts,
                                                int(bool(msg.is_bigendian)), out.data_ptr(), s), None, "pp_unpack_points")
    return out


def _box_corners_bev(boxes):
    """center_to_corner_box2d(xy, lw, r) (box_np_ops.py:81-119): f32[N,4,2] in the reference's corner order."""
    dims = boxes[:, [3, 4]]
    norm = np.array([[-0.5, -0.5], [-0.5, 0.5], [0.5, 0.5], [0.5, -0.5]], dtype=dims.dtype)
    corners = dims.reshape(-1, 1, 2) * norm.reshape(1, 4, 2)
    s, c = np.sin(boxes[:, 6]), np.cos(boxes[:, 6])
    corners = np.einsum('aij,jka->aik', corners, np.stack([[c, s], [-s, c]]))
    return corners + boxes[:, [0, 1]].reshape(-1, 1, 2)


def gt_in_range(boxes, bv_range):
    """filter_gt_box_outside_range (box_np_ops.py:6-16): keep a box when any of its four BEV corners lies strictly inside
    the range rectangle (points_in_convex_polygon_jit, clockwise)."""
    x0, y0, x1, y1 = [np.asarray(v, dtype=boxes.dtype) for v in bv_range]
    poly = np.array([[x0, y0], [x0, y1], [x1, y1], [x1, y0]], dtype=boxes.dtype)
    vec = poly - poly[[3, 0, 1, 2]]
    pts = _box_corners_bev(boxes).reshape(-1, 2)
    inside = np.ones(pts.shape[0], bool)
    for k in range(4):
        cross = vec[k, 1] * (poly[k, 0] - pts[:, 0]) - vec[k, 0] * (poly[k, 1] - pts[:, 1])
        inside &= cross < 0
    return inside.reshape(-1, 4).any(1)


def gt_from_annos(annos, detect_class, detection_range):
    """GenericDataset.__getitem__'s ground truth without augmentation (dataset.py:108-140): class filter, 1-based ids in
    detect_class order, float32 (x,y,z,l,w,h,r) boxes, boxes whose four BEV corners all lie outside the range dropped, then
    limit_period(r, 0.5, 2 pi).  Returns (gt_classes i32[G], gt_boxes f32[G,7])."""
    names = np.asarray(annos["name"])
    keep = np.array([n in detect_class for n in names], dtype=np.bool_)
    cls = np.array([detect_class.index(n) + 1 for n in names[keep]], dtype=np.int32)
    boxes = np.concatenate([np.asarray(annos["location"])[keep].reshape(-1, 3), np.asarray(annos["dimensions"])[keep].reshape(-1, 3),
                            np.asarray(annos["rotation_y"])[keep].reshape(-1, 1)], axis=1).astype(np.float32)
    rng = np.asarray(detection_range, dtype=np.float32)[[0, 1, 3, 4]]
    m = gt_in_range(boxes, rng)
    boxes, cls = boxes[m], cls[m]
    boxes[:, 6] = boxes[:, 6] - np.floor(boxes[:, 6] / (2 * np.pi) + 0.5) * (2 * np.pi)
    return cls, boxes


# create_info.py:180: the box grows by this (l, w, h) before the second count
DIFFICULTY_EXTRA = (1.2, 0.5, 8.0)


def point_counts(points, boxes, config=None):
    """add_difficulty_to_annos_v2 (create_info.py:159-183): per lidar box (x, y, z, l, w, h, r) the points inside it
    (annos["num_points"]) and inside the box grown by (1.2, 0.5, 8) (annos["difficulty"]), counted on the device (pp_gt_count) in
    float32.  points f32[N,4], boxes [M,7], numpy or device tensors -> two i32[M] numpy arrays.  config: the engine's, default the
    augmentation's (a live engine, else the shipped eight_20cm one)."""
    from .framework.augmentation import _engine
    eng = engine_for(config) if config is not None else _engine()
    as_dev = lambda a: (a.to(eng.device, torch.float32).contiguous() if isinstance(a, torch.Tensor)
                        else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(eng.device))
    pts, bx = as_dev(points).reshape(-1, 4), as_dev(boxes).reshape(-1, 7)
    off_p, off_b = [0, int(pts.shape[0])], [0, int(bx.shape[0])]
    num = eng.gt_count(pts, off_p, bx, off_b)
    diff = eng.gt_count(pts, off_p, bx, off_b, DIFFICULTY_EXTRA)
    host = torch.stack([num, diff]).cpu().numpy()
    return host[0], host[1]


def sequence_loss(config, clouds, gts, batch=16, nms_mode=0):
    """Validation loss over a labelled sequence: clouds (numpy f32[N,4] or .bin paths) and gts [(gt_classes, gt_boxes)] per frame
    go through pp_infer_batch and pp_batch_loss `batch` frames at a time, one D2H of the loss terms per pass.  Returns
    (per-frame dicts of the reference's six loss keys as floats, framework.metrics.Metric over the whole sequence)."""
    from .framework.loss_generator import combine_terms
    from .framework.metrics import Metric
    eng = engine_for(config)
    batch = max(1, min(int(batch), eng.max_batch))
    metric = Metric(config)
    losses = []
    was = eng.head_defer
    eng.set_head_defer(False)  # batch_loss reads the full box / dir tensors after every pass: do not pay for both heads
    try:
        for i0 in range(0, len(clouds), batch):
            group = []
            for c in clouds[i0:i0 + batch]:
                pts = read_velodyne(c) if isinstance(c, (str, os.PathLike)) else np.ascontiguousarray(c, dtype=np.float32)
                group.append(torch.from_numpy(pts).to(eng.device, non_blocking=True))
            nb = len(group)
            eng.infer_batch(group, nms_mode=nms_mode)
            g = gts[i0:i0 + nb]
            off = np.concatenate([[0], np.cumsum([len(np.asarray(c)) for c, _ in g])]).tolist()
            cls = torch.from_numpy(np.concatenate([np.asarray(c, np.int32).reshape(-1) for c, _ in g])).to(eng.device)
            box = torch.from_numpy(np.concatenate([np.asarray(b, np.float32).reshape(-1, 7) for _, b in g])).to(eng.device)
            terms = eng.batch_loss(box, cls, off, nb).cpu().numpy()
            losses += [combine_terms(terms[f:f + 1]) for f in range(nb)]
            metric.update_counts(terms)
    finally:
        eng.set_head_defer(was)
    return losses, metric
