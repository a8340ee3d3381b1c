"""framework.dataset: GenericDataset (reference dataset.py:13-175), the training / evaluation loader, and InferData (:199-231):
voxelise + anchor mask -> example dict.  The augmentation, voxeliser, anchor mask and target assignment run on the device; the host
keeps the random draws (framework.augmentation.draw_frame) and the file reads.  CUDA does not survive fork: use num_workers=0 with a
torch DataLoader, or get_batch, which runs the augmentation of B frames as one set of launches (voxeliser and anchor mask per
frame, target assignment once).

config["gt_sampler"] (framework.gt_sampler) switches ground-truth database sampling on for training with augm=True: after the class
filter and in front of the chain, recorded objects are selected (greedy collision rejection) and pasted into the cloud on the device;
the accepted boxes, classes, names and difficulty are appended behind the frame's own (valid True; the frame's own boxes keep the
dataset.py:126-127 quirk) and the unchanged chain runs on the new cloud and boxes, so noise_per_object moves pasted objects too and the
permutation covers the new point count.  Cost: one extra small D2H per batch (accept flags, candidate rows, output sizes) in device
mode; numpy mode runs select / paste frame by frame, because a frame's draw_frame draws need its new point and box counts and must
follow its own sampling draws in the stream.  Without the key nothing of this is entered."""
import time
from pathlib import Path

import numpy as np
import torch

from .. import kitti_io
from ..engine import engine_for
from . import augmentation as agm
from . import gt_sampler as gts


class InferData:
    def __init__(self, config, voxel_generator, anchor_assigner, dtype=torch.float32):
        self.voxel_generator = voxel_generator
        self.anchor_assigner = anchor_assigner
        self.grid_size = config['grid_size']
        self.create_mask_gpu = config.get('create_mask_gpu', 1) == 1
        self.dtype = dtype
        self.voxel_time = 0.0
        self.mask_time = 0.0
        self.convert_time = 0.0
        self.device = config['device']
        self._config = config
        self.profile_stages = True  # voxel_time / mask_time / convert_time are per-stage wall times like the reference's (:208-229)

    def get(self, points, toTorch=True):
        eng = engine_for(self._config)
        sync = torch.cuda.synchronize if self.profile_stages else (lambda: None)
        start = time.time()
        # the reference converts to device tensors LAST (example_convert_to_torch, utils.py:7-20); here the cloud goes up
        # first and everything after it stays on the device -- its upload is what convert_time measures
        if isinstance(points, torch.Tensor):
            pts = points.to(eng.device, torch.float32).contiguous()
        else:
            pts = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(eng.device)
        sync()
        convert_time = time.time()
        voxels, coors, npts, num = eng.voxelize(pts)
        p = int(num.item())  # the one unavoidable sync: the reference's example carries exact-length tensors
        voxel_time = time.time()
        mask = eng.anchor_mask(coors, num).view(torch.bool)
        sync()
        mask_time = time.time()
        example = {'voxels': voxels[:p], 'coordinates': coors[:p], 'num_points_per_voxel': npts[:p],
                   'anchors_mask': mask[None, :]}
        self.convert_time += convert_time - start
        self.voxel_time += voxel_time - convert_time
        self.mask_time += mask_time - voxel_time
        if not toTorch:
            example = {k: v.cpu().numpy() for k, v in example.items()}
        return example


class GenericDataset:
    def __init__(self, config, info_paths, voxel_generator, anchor_assigner, training=True, augm=True, *, rng="numpy", seed=None):
        if rng not in ("numpy", "device"):
            raise ValueError("GenericDataset: rng must be 'numpy' (the reference's global np.random stream) or 'device'")
        self.data_root = Path(config['data_root'])
        self.infos = kitti_io.load_infos(self.data_root, info_paths)
        kitti_io.remap_classes(self.infos)  # dataset.py:45-77: drop boxes without points, map onto vehicle / pedestrian / cyclist
        self.num_point_features = config['num_point_features']
        self.voxel_generator = voxel_generator
        self.anchor_assigner = anchor_assigner
        self.detect_class = config['detect_class']
        self.augm_class = config['detect_class']
        self.detection_range = np.asarray(config['detection_range'], dtype=np.float32)
        self.grid_size = config['grid_size']
        self.training = training
        self.augm = augm
        self.rng = rng
        self.epoch = 0
        self._config = config
        # numpy mode: seed seeds the global stream, as np.random.seed before the reference's loader; device mode: the Philox key
        self.seed = 0 if seed is None else int(seed)
        if seed is not None and rng == "numpy":
            np.random.seed(seed)
        self.sampler = None
        if training and augm and 'gt_sampler' in config:
            self.sampler = gts.GtSampler(config, gts.GtDatabase.load(self.data_root / config['gt_sampler']['database']))

    def __len__(self):
        return len(self.infos)

    def set_epoch(self, e):
        """Device mode: the epoch is part of every frame's key, so each epoch draws afresh (numpy mode: the stream moves on)."""
        self.epoch = int(e)

    def _engine(self):
        # the voxeliser the caller built is the one that runs: its config dict carries the engine (VoxelGenerator.generate uses it)
        return engine_for(getattr(self.voxel_generator, "_config", self._config))

    def _read(self, idx):
        """Host part of __getitem__ for one frame: the cloud, the calibration entries, the class-filtered ground truth and the draws,
        in the reference's order of np.random use."""
        info = self.infos[idx]
        points = kitti_io.read_velodyne(self.data_root / info['velodyne_path'], self.num_point_features)
        ex = {'image_idx': info["image_idx"], 'image_shape': info["img_shape"], 'rect': info['calib/R0_rect'].astype(np.float32),
              'Trv2c': info['calib/Tr_velo_to_cam'].astype(np.float32), 'P2': info['calib/P2'].astype(np.float32)}
        gt = None
        if self.training:
            annos = info['annos']
            names = annos["name"]
            gt_class_mask = np.array([n in self.detect_class for n in names], dtype=np.bool_)
            gt_names = names[gt_class_mask]
            gt_classes = np.array([self.detect_class.index(n) + 1 for n in gt_names], dtype=np.int32)
            gt_boxes = np.concatenate([annos["location"][gt_class_mask], annos["dimensions"][gt_class_mask],
                                       annos["rotation_y"][gt_class_mask][..., np.newaxis]], axis=1).astype(np.float32)
            # quirk of dataset.py:126-127: the class mask of ALL annotations is the valid_mask of the filtered boxes (entry i for box i)
            augm_class_mask = np.array([n in self.augm_class for n in names], dtype=np.bool_)
            gt = dict(names=gt_names, classes=gt_classes, boxes=gt_boxes, difficulty=annos["difficulty"][gt_class_mask],
                      valid=augm_class_mask[:gt_boxes.shape[0]])
        draws = None
        if self.rng == "numpy":
            if self.sampler is not None:  # the sampling draws first, then select / paste: draw_frame needs the new counts
                rows = self.sampler.draw_numpy(gt['classes'])
                points, gt, gt['sample'] = gts.paste_frames(self._engine(), self.sampler, [points], [gt], cand_rows=[rows])[0]
            draws = agm.draw_frame(points.shape[0], 0 if gt is None else gt['boxes'].shape[0], self.training, self.augm)
        return ex, points, gt, draws, idx

    def _sample_device(self, frames):
        """Device mode: select -> paste for the frames of one batch as one set of launches, keyed by (seed, epoch, index)."""
        if self.sampler is None or self.rng != "device":
            return frames
        res = gts.paste_frames(self._engine(), self.sampler, [f[1] for f in frames], [f[2] for f in frames],
                               draw=(self.seed, self.epoch, [f[4] for f in frames]))
        out = []
        for f, (points, gt, record) in zip(frames, res):
            gt['sample'] = record
            out.append((f[0], points, gt, f[3], f[4]))
        return out

    def export_samples(self, indices):
        """Test hook: per frame the sampling record of paste_frames -- the frame's own boxes, the candidates' database rows in
        decision order, the accept flags -- plus the cloud and boxes as they enter the chain.  numpy mode consumes the stream as
        __getitem__ does."""
        if self.sampler is None:
            raise ValueError("export_samples: the dataset has no gt_sampler")
        frames = self._sample_device([self._read(i) for i in indices])
        return [dict(f[2]['sample'], points=f[1].cpu().numpy(), gt_boxes=f[2]['boxes'].copy(), gt_classes=f[2]['classes'].copy(),
                     valid=f[2]['valid'].copy()) for f in frames]

    def _run(self, frames):
        """Device part for the frames of one batch: one set of augmentation launches, then per frame the voxeliser and the anchor
        mask, one D2H of the pillar counts, kept counts and keep flags, and one assign_batch.  Returns per-frame device results."""
        eng = self._engine()
        dev = eng.device
        nb = len(frames)
        frames = self._sample_device(frames)
        pt_off = np.concatenate([[0], np.cumsum([f[1].shape[0] for f in frames])]).astype(np.int64).tolist()
        if isinstance(frames[0][1], torch.Tensor):  # pasted clouds are on the device already
            pts = torch.cat([f[1] for f in frames])
        else:
            pts = torch.from_numpy(np.ascontiguousarray(np.concatenate([f[1] for f in frames]), dtype=np.float32)).to(dev)
        if self.training:
            gts = [f[2] for f in frames]
            box_off = np.concatenate([[0], np.cumsum([g['boxes'].shape[0] for g in gts])]).astype(np.int64).tolist()
            boxes = torch.from_numpy(np.concatenate([g['boxes'] for g in gts]).reshape(-1, 7)).to(dev)
            classes = torch.from_numpy(np.concatenate([g['classes'] for g in gts]).astype(np.int32)).to(dev)
            valid = torch.from_numpy(np.concatenate([g['valid'] for g in gts]).astype(np.uint8)).to(dev)
            bv_range = self.detection_range[[0, 1, 3, 4]]
            draws = self._device_draws(eng, frames, box_off) if self.rng == "device" else [f[3] for f in frames]
            pts, out_box, out_cls, keep, kept, _ = agm.run_frames(eng, pts, pt_off, boxes, classes, valid, box_off, draws, bv_range)
        res = []
        for f in range(nb):
            voxels, coors, npts, num = eng.voxelize(pts[pt_off[f]:pt_off[f + 1]])
            mask = self.anchor_assigner.create_mask_device(coors, num).view(torch.uint8)
            res.append(dict(points=pts[pt_off[f]:pt_off[f + 1]], voxels=voxels, coors=coors, npts=npts, num=num, mask=mask))
        counts = [r['num'] for r in res]
        if self.training:
            counts += [kept, keep.to(torch.int32)]
        host = torch.cat(counts).cpu().numpy()  # the one D2H of the batch
        for f in range(nb):
            res[f]['p'] = int(host[f])
        if self.training:
            kept_h, keep_h = host[nb:2 * nb], host[2 * nb:].astype(bool)
            gl, gc = [], []
            for f in range(nb):
                k = int(kept_h[f])
                g = frames[f][2]
                km = keep_h[box_off[f]:box_off[f + 1]]
                res[f]['gt_boxes'] = out_box[box_off[f]:box_off[f] + k]
                res[f]['gt_classes'] = out_cls[box_off[f]:box_off[f] + k]
                res[f]['annos_host'] = dict(gt_names=g['names'][km], difficulty=g['difficulty'][km], gt_classes=g['classes'][km])
                gl.append((res[f]['gt_classes'], res[f]['gt_boxes']))
            masks = torch.stack([r['mask'] for r in res])
            labels, tgt, ow, dirt = self.anchor_assigner.assign_batch(gl, masks)
            for f in range(nb):
                res[f].update(labels=labels[f], bbox_targets=tgt[f], bbox_outside_weights=ow[f], dir_targets=dirt[f])
        return res

    def _device_draws(self, eng, frames, box_off):
        return agm.draw_device(eng, self.seed, self.epoch, [f[4] for f in frames], box_off, self.training, self.augm)

    def export_params(self, indices):
        """Test hook (device mode): the drawn records of these frames as host draw_frame dicts, the permutation included."""
        if self.rng != "device" or not self.training:
            raise ValueError("export_params: only a training dataset in device mode draws on the device")
        frames = self._sample_device([self._read(i) for i in indices])
        eng = self._engine()
        box_off = np.concatenate([[0], np.cumsum([f[2]['boxes'].shape[0] for f in frames])]).astype(np.int64).tolist()
        pt_off = np.concatenate([[0], np.cumsum([f[1].shape[0] for f in frames])]).astype(np.int64).tolist()
        return agm.export_device_draws(eng, self._device_draws(eng, frames, box_off), pt_off)

    def __getitem__(self, idx):
        frame = self._read(idx)
        ex = frame[0]
        r = self._run([frame])[0]
        p = r['p']
        if self.training:
            a = r['annos_host']
            ex['annos'] = {'gt_classes': a['gt_classes'], 'gt_boxes': r['gt_boxes'].cpu().numpy(), 'difficulty': a['difficulty'],
                           'gt_names': a['gt_names']}
        ex['voxels'] = r['voxels'][:p].cpu().numpy()
        ex['coordinates'] = r['coors'][:p].cpu().numpy()
        ex['num_points_per_voxel'] = r['npts'][:p].cpu().numpy()
        ex['anchors_mask'] = r['mask'].view(torch.bool).cpu().numpy()
        ex['points'] = r['points'].cpu().numpy()
        if self.training:
            for k in ('labels', 'bbox_targets', 'dir_targets', 'bbox_outside_weights'):
                ex[k] = r[k].cpu().numpy()
        return ex

    def get_batch(self, indices):
        """B frames through one set of augmentation launches, collated as merge_second_batch would (device tensors): voxels and
        num_points_per_voxel concatenated, coordinates with the frame index appended as the last column, anchors_mask and the
        targets stacked, points as one concatenation plus `points_offsets` i64[B+1] (the reference's np.stack raises on ragged
        clouds).  Draws are made frame by frame in index order, so the stream and every frame equal B calls of __getitem__."""
        frames = [self._read(i) for i in indices]
        res = self._run(frames)
        dev = res[0]['voxels'].device
        out = {k: np.stack([f[0][k] for f in frames]) for k in ('image_idx', 'image_shape', 'rect', 'Trv2c', 'P2')}
        out['voxels'] = torch.cat([r['voxels'][:r['p']] for r in res])
        out['num_points_per_voxel'] = torch.cat([r['npts'][:r['p']] for r in res])
        out['coordinates'] = torch.cat([torch.nn.functional.pad(r['coors'][:r['p']], (0, 1), value=f) for f, r in enumerate(res)])
        out['anchors_mask'] = torch.stack([r['mask'].view(torch.bool) for r in res])
        out['points'] = torch.cat([r['points'] for r in res])
        out['points_offsets'] = torch.tensor(np.concatenate([[0], np.cumsum([r['points'].shape[0] for r in res])]), dtype=torch.int64,
                                             device=dev)
        if self.training:
            for k in ('labels', 'bbox_targets', 'dir_targets', 'bbox_outside_weights'):
                out[k] = torch.stack([r[k] for r in res])
            out['annos'] = [dict(r['annos_host'], gt_boxes=r['gt_boxes']) for r in res]
        return out
