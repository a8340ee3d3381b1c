"""framework.loss_generator.LossGenerator (reference loss_generator.py:26-253): the NormByNumPositives detection loss -- sigmoid focal
classification (gamma 2, alpha 0.25), smooth-L1 regression (sigma 3, sin difference on the angle code), 2-way softmax direction
loss -- computed by pp_target_loss (assign.hip) with a deterministic fp64 reduction.  Forward only: the values serve validation."""
import numpy as np
import torch

from ..engine import engine_for

# weights of loss_generator.py:16-24
LOC_WEIGHT, CLS_WEIGHT, DIR_WEIGHT = 0.25, 1.0, 0.2
KEYS = ("loss", "cls_pos_loss", "cls_neg_loss", "dir_loss", "cls_loss", "loc_loss")


def combine_terms(terms):
    """Per-frame terms f64[B, PP_LOSS_TERMS] (host numpy) -> the reference's six batch values as Python floats."""
    t = np.asarray(terms, dtype=np.float64).reshape(-1, terms.shape[-1])
    B = t.shape[0]
    loc = t[:, 1].sum() / B * LOC_WEIGHT
    cpos, cneg = t[:, 2].sum() / B, t[:, 3].sum() / B
    cls = (t[:, 2] + t[:, 3]).sum() / B * CLS_WEIGHT
    dirl = t[:, 4].sum() / B
    return dict(loss=loc + cls + DIR_WEIGHT * dirl, cls_pos_loss=cpos, cls_neg_loss=cneg, dir_loss=dirl, cls_loss=cls, loc_loss=loc)


def _dev(x, dtype, device):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(x)).to(device=device, dtype=dtype)


class LossGenerator:
    def __init__(self, config):
        self._box_code_size = config['box_code_size']
        self._config = config
        self.device = engine_for(config).device
        self.last_terms = None  # f64[B, PP_LOSS_TERMS] of the last generate (metric counts included)

    def generate(self, preds_dict, example):
        """preds_dict: cls_preds [B,A(,1)], box_preds [B,A,7], dir_preds [B,A,2]; example: labels [B,A], bbox_targets [B,A,7],
        dir_targets [B,A] (numpy as the reference's DataLoader yields them, or torch).  Returns the reference's six keys as 0-d
        float32 tensors on the device."""
        eng = engine_for(self._config)
        dev = eng.device
        labels = _dev(example['labels'], torch.int32, dev)
        B = int(labels.shape[0])
        labels = labels.reshape(B, -1)
        tgt = _dev(example['bbox_targets'], torch.float32, dev).reshape(B, -1, self._box_code_size)
        dirt = _dev(example['dir_targets'], torch.int32, dev).reshape(B, -1)
        cls = _dev(preds_dict['cls_preds'], torch.float32, dev).reshape(B, -1)
        box = _dev(preds_dict['box_preds'], torch.float32, dev).reshape(B, -1, self._box_code_size)
        dr = _dev(preds_dict['dir_preds'], torch.float32, dev).reshape(B, -1, 2)
        terms = torch.cat([eng.target_loss(cls[i:i + k], box[i:i + k], dr[i:i + k], labels[i:i + k], tgt[i:i + k], dirt[i:i + k])
                           for i in range(0, B, eng.max_batch) for k in [min(eng.max_batch, B - i)]])
        self.last_terms = terms
        vals = combine_terms(terms.cpu().numpy())
        return {k: torch.tensor(vals[k], dtype=torch.float32, device=dev) for k in KEYS}
