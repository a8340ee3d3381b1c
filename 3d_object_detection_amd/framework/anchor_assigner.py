"""framework.anchor_assigner.AnchorAssigner (reference anchor_assigner.py:220-457): anchor tables, the occupied-anchor mask and
the training targets (`assign`), all on the device (anchor_mask.hip, assign.hip)."""
import numpy as np
import torch

from ..engine import class_table_of, engine_for


class AnchorAssigner:
    def __init__(self, config):
        # the reference overwrites detect_class and adds the per-class dicts (:222-245); a config with its own
        # `class_table` (build-side extension, engine.class_table_of) keeps its classes
        names, table = class_table_of(config)
        config['detect_class'] = list(names)
        self.detect_class = config['detect_class']
        fm = [int(config['grid_size'][0]) // 2, int(config['grid_size'][1]) // 2, 1]
        for name in names:
            t = table[name]
            config[name] = dict(sizes=[list(s) for s in t['sizes']], rotations=list(t['rotations']),
                                feature_map_size=[list(fm) for _ in t['sizes']],
                                matched_threshold=t.get('matched_threshold', 0.6), unmatched_threshold=t.get('unmatched_threshold', 0.45))
        self.anchor_offsets = config['detection_offset']
        self.grid_size = config['grid_size']
        self.box_code_size = config['box_code_size']
        self._config = config
        eng = engine_for(config)
        self.anchors = eng.anchors_np
        self.anchors_bv = eng.anchors_bv
        self.anchors_coors = eng.rects_np
        self.class_masks = eng.class_masks
        self.matched_threshold = np.concatenate(
            [np.full(e - s, table[n].get('matched_threshold', 0.6), np.float32) for n, (s, e) in self.class_masks.items()])
        self.unmatched_threshold = np.concatenate(
            [np.full(e - s, table[n].get('unmatched_threshold', 0.45), np.float32) for n, (s, e) in self.class_masks.items()])

    def create_mask_device(self, coors, num):
        """coors i32[>=P,3] cuda, num i32[1] cuda -> bool[A] cuda."""
        return engine_for(self._config).anchor_mask(coors, num).view(torch.bool)

    def create_mask(self, coors, grid_size=None, voxel_size=None, offset=None, gpu=True):
        """numpy coors in, numpy bool[A] out (the reference's signature; gpu flag is ignored --
        there is only the device path)."""
        eng = engine_for(self._config)
        if isinstance(coors, torch.Tensor):
            co = coors.to(eng.device, torch.int32).contiguous()
        else:
            co = torch.from_numpy(np.ascontiguousarray(coors, dtype=np.int32)).to(eng.device)
        if co.shape[0] > eng.max_voxels:
            raise ValueError("more pillars than max_voxels")
        mask = eng.anchor_mask(co, eng.num_tensor(co.shape[0])).view(torch.bool)
        return mask if isinstance(coors, torch.Tensor) else mask.cpu().numpy()

    def assign(self, gt_classes_all, gt_boxes_all, anchors_mask_all):
        """The reference's assign (anchor_assigner.py:337-457) through pp_assign_targets: gt classes (1-based, detect_class order)
        [G], boxes [G,7], anchor mask [A] -> labels int32[A], bbox_targets float32[A,7], bbox_outside_weights float32[A],
        dir_cls_targets int32[A].  numpy in gives numpy out; torch tensors in give device tensors out."""
        as_np = not isinstance(gt_boxes_all, torch.Tensor)
        out = self.assign_batch([(gt_classes_all, gt_boxes_all)], self._dev(anchors_mask_all, torch.uint8).reshape(1, -1))
        out = tuple(t[0] for t in out)
        return tuple(t.cpu().numpy() for t in out) if as_np else out

    def assign_batch(self, gt_list, masks):
        """nb frames in one pp_assign_targets call: gt_list [(gt_classes [G_i], gt_boxes [G_i,7])] (numpy or torch), masks [nb,A]
        -> device tensors labels i32[nb,A], bbox_targets f32[nb,A,7], outside weights f32[nb,A], dir targets i32[nb,A]."""
        eng = engine_for(self._config)
        cls = [self._dev(c, torch.int32).reshape(-1) for c, _ in gt_list]
        box = [self._dev(b, torch.float32).reshape(-1, 7) for _, b in gt_list]
        off = np.concatenate([[0], np.cumsum([int(c.shape[0]) for c in cls])]).tolist()
        return eng.assign_targets(self._dev(masks, torch.uint8), torch.cat(box).contiguous(), torch.cat(cls).contiguous(), off)

    def _dev(self, x, dtype):
        eng = engine_for(self._config)
        if isinstance(x, torch.Tensor):
            return x.to(eng.device).to(dtype).contiguous()
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(torch.empty(0, dtype=dtype).numpy().dtype))).to(eng.device)
