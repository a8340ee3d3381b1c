"""framework.loss_generator.LossGenerator (reference loss_generator.py:26-253): the NormByNumPositives detection loss -- sigmoid focal
classification (gamma 2, alpha 0.25), smooth-L1 regression (sigma 3, sin difference on the angle code), 2-way softmax direction
loss -- computed by pp_target_loss (assign.hip) with a deterministic fp64 reduction.  When a prediction requires grad, the `loss` key
carries a grad_fn whose backward is pp_target_loss_grad (train.hip): the gradient with respect to the three head outputs.  The
other five keys are values only."""
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


class _LossFunction(torch.autograd.Function):
    """`loss` of LossGenerator.generate: forward = the value of the pp_target_loss path, backward = pp_target_loss_grad per chunk of
    at most max_batch frames, each scaled by the upstream gradient over the WHOLE batch size."""

    @staticmethod
    def forward(ctx, eng, value, cls, box, dr, labels, tgt, dirt):
        ctx.eng = eng
        ctx.save_for_backward(cls, box, dr, labels, tgt, dirt)
        return value.clone()

    @staticmethod
    def backward(ctx, grad):
        cls, box, dr, labels, tgt, dirt = ctx.saved_tensors
        eng, B = ctx.eng, int(labels.shape[0])
        scale = float(grad)
        parts = [eng.target_loss_grad(cls[i:i + k], box[i:i + k], dr[i:i + k], labels[i:i + k], tgt[i:i + k], dirt[i:i + k], scale, B)
                 for i in range(0, B, eng.max_batch) for k in [min(eng.max_batch, B - i)]]
        dcls, dbox, ddir = (torch.cat([p[j] for p in parts]) for j in range(3))
        return None, None, dcls.reshape(cls.shape), dbox.reshape(box.shape), ddir.reshape(dr.shape), None, None, None


class LossGenerator:
    def __init__(self, config):
        self._box_code_size = config['box_code_size']
        self._config = config
        self.device = engine_for(config).device
        self.last_terms = None  # f64[B, PP_LOSS_TERMS] of the last generate (metric counts included)

    def generate(self, preds_dict, example):
        """preds_dict: cls_preds [B,A(,1)], box_preds [B,A,7], dir_preds [B,A,2]; example: labels [B,A], bbox_targets [B,A,7],
        dir_targets [B,A] (numpy as the reference's DataLoader yields them, or torch).  Returns the reference's six keys as 0-d
        float32 tensors on the device.  With a prediction that requires grad, `loss` is differentiable (same value, bit for bit)."""
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
        out = {k: torch.tensor(vals[k], dtype=torch.float32, device=dev) for k in KEYS}
        if torch.is_grad_enabled() and any(isinstance(preds_dict[k], torch.Tensor) and preds_dict[k].requires_grad
                                           for k in ('cls_preds', 'box_preds', 'dir_preds')):
            out["loss"] = _LossFunction.apply(eng, out["loss"], cls, box, dr, labels, tgt, dirt)
        return out
