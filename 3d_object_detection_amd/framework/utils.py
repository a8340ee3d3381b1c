"""framework.utils (reference utils.py:7-48): host->device conversion of an example dict and the batch collation."""
from collections import defaultdict

import numpy as np
import torch


def example_convert_to_torch(example, dtype=torch.float32, device=torch.device("cuda:0")):
    out = {}
    for k, v in example.items():
        if k in ["voxels"]:
            out[k] = torch.as_tensor(v, dtype=dtype, device=device)
        elif k in ["coordinates", "num_points_per_voxel", "voxel_num"]:
            out[k] = torch.as_tensor(v, dtype=torch.int32, device=device)
        elif k in ["anchors_mask"]:
            out[k] = torch.as_tensor(v, dtype=torch.bool, device=device)
        else:
            out[k] = v
    return out


def merge_second_batch(batch_list, _unused=False):
    """The reference's collate function (utils.py:23-48), numpy in and out: voxels / num_points_per_voxel concatenated,
    coordinates with the frame index appended as a last column when there are several frames, everything else np.stack'ed."""
    example_merged = defaultdict(list)
    for example in batch_list:
        for k, v in example.items():
            example_merged[k].append(v)
    ret = {}
    for key, elems in example_merged.items():
        if key in ['voxels', 'num_points_per_voxel', 'match_indices_num']:
            ret[key] = np.concatenate(elems, axis=0)
        elif key == 'coordinates':
            if len(batch_list) > 1:
                ret[key] = np.concatenate([np.pad(c, ((0, 0), (0, 1)), mode='constant', constant_values=i) for i, c in enumerate(elems)],
                                          axis=0)
            else:
                ret[key] = np.concatenate(elems, axis=0)
        else:
            ret[key] = np.stack(elems, axis=0)
    return ret
