"""networks.pointpillars8_shared.PointPillars (reference pointpillars8_shared.py:346-382): the eager
network with the InstanceNorm backbone, running PFN / scatter / RPN / head as HIP kernels.

Training surface: head-only fine-tuning.  The backbone (PFN, scatter, RPN) is FROZEN: it has no backward pass, and
parameters() yields the six tensors of the anchor head only.  train() makes them require grad; heads(x) then records a
torch.autograd.Function whose backward is pp_head_backward (csrc/train.hip)."""
import time

import numpy as np
import torch

from ..engine import engine_for
from .init import init_state_dict

HEAD_KEYS = ("heads.conv_cls.weight", "heads.conv_cls.bias", "heads.conv_box.weight", "heads.conv_box.bias",
             "heads.conv_dir.weight", "heads.conv_dir.bias")


class _HeadFunction(torch.autograd.Function):
    """SharedHead.forward as pp_head, its backward as pp_head_backward.  The six parameters are inputs only so that autograd
    routes their gradients; the forward reads the engine's packed copy of them (PointPillars uploads it beforehand)."""

    @staticmethod
    def forward(ctx, eng, x, *params):
        ctx.eng = eng
        ctx.save_for_backward(x)
        return eng.head(x)

    @staticmethod
    def backward(ctx, gcls, gbox, gdir):
        (x,) = ctx.saved_tensors
        eng = ctx.eng
        nb = x.shape[0]
        zeros = lambda g, n: torch.zeros((nb, eng.A, n), dtype=torch.float32, device=x.device) if g is None else g.contiguous()  # noqa: E731
        g, dx = eng.head_backward(x, zeros(gcls, 1), zeros(gbox, 7), zeros(gdir, 2), need_dx=ctx.needs_input_grad[1])
        return (None, dx) + tuple(g[k] if ctx.needs_input_grad[2 + i] else None for i, k in enumerate(HEAD_KEYS))


class PointPillars:
    _norm = "instance"

    def __init__(self, config):
        self.device = config['device']
        self._config = config
        config['_pp_norm'] = self._norm
        self._eng = engine_for(config, self._norm)
        self._sd = None
        self._params = {}            # the six head tensors as device Parameters (parameters())
        self._uploaded = None        # their _version numbers at the last upload into the engine
        self.training = False
        self._trained = False        # the head has been stepped since load_state_dict
        self.profile_stages = True  # the reference synchronises after every stage (:365-374)
        self.pfn_time, self.rpn_time, self.scatter_time, self.heads_time = 0.0, 0.0, 0.0, 0.0
        # like nn.Module construction, start from random initial weights
        self.load_state_dict(init_state_dict(0, norm=self._norm))

    # nn.Module-style surface used by train.py:196-205
    def to(self, device):
        return self

    def eval(self):
        return self.train(False)

    def train(self, mode=True):
        """Head-only training mode: the six head parameters require grad (the backbone stays frozen: it has no backward), and
        forward() accepts a batch of several frames.  eval() / train(False) restores the inference behaviour."""
        self.training = bool(mode)
        for p in self._params.values():
            p.requires_grad_(self.training)
        return self

    def named_parameters(self):
        """The trainable tensors: heads.conv_{cls,box,dir}.{weight,bias} on the device.  Everything before the head is frozen."""
        return iter(self._params.items())

    def parameters(self):
        return iter(self._params.values())

    def zero_grad(self, set_to_none=True):
        for p in self._params.values():
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def _sync_head(self):
        """An optimizer stepped (a parameter's _version moved since the last upload): rewrite the engine's packed head in place."""
        ver = tuple(p._version for p in self._params.values())
        if ver != self._uploaded:
            self._eng.update_head_weights(self._params)
            self._uploaded = ver

    def half(self):
        """The reference deploys FP16 TensorRT engines (framework/trt_utils.py:30, networks/pointpillars8_trt.py:208-223,295-314).
        Here: fp16 MFMA operands for every convolution, upsampler and the head, fp32 accumulation, activations still fp32 in
        HBM; tolerance table in DESIGN.md.  The parity contract (<= 1e-3 vs the fp32 reference) is stated for float() / the
        default (and is also met by precision("bf16x3"))."""
        return self.precision("fp16")

    def float(self):
        return self.precision("fp32")

    def precision(self, mode):
        """ "fp32" | "bf16x3" (split-bf16: fp32-equivalent on the bf16 MFMAs) | "fp16" | "bf16" | "fp16s" (fp16 operands and fp16 tensors)."""
        self._eng.set_precision(mode)
        if self._trained or self._head_moved():
            self._uploaded = ()  # a change of mode packs the loaded weights again: the trained head is uploaded at the next heads()
        return self

    def _head_moved(self):
        return self._uploaded is not None and tuple(p._version for p in self._params.values()) != self._uploaded

    def state_dict(self):
        """The loaded tensors, the head's six with their CURRENT values (after optimizer steps)."""
        sd = dict(self._sd)
        if self._head_moved() or self._trained:
            for k, p in self._params.items():
                sd[k] = p.detach().cpu().numpy().reshape(self._sd[k].shape)
        return sd

    def load_state_dict(self, sd, strict=True):
        self._sd = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in sd.items()}
        self._eng.load_state_dict(self._sd)
        self._params = {k: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(self._sd[k], dtype=np.float32)).to(self._eng.device),
                                              requires_grad=self.training) for k in HEAD_KEYS if k in self._sd}
        self._uploaded = tuple(p._version for p in self._params.values())
        self._trained = False
        return self

    def _sync(self):
        if self.profile_stages:
            torch.cuda.synchronize()
        return time.time()

    def _forward_frames(self, example):
        """Several frames collated by merge_second_batch (coordinates carry the frame index as their last column): each frame runs
        the frozen PFN / scatter / backbone, the rpn outputs are stacked and the head runs on the batch."""
        eng = self._eng
        coors = example["coordinates"]
        frame = coors[:, -1]
        nb = int(frame.max().item()) + 1 if coors.shape[0] else 1
        if not 1 <= nb <= eng.max_batch:
            raise ValueError(f"forward: {nb} frames in the batch, max_batch is {eng.max_batch}")
        rpn = []
        with torch.no_grad():
            for f in range(nb):
                sel = frame == f
                c = coors[sel][:, :-1].contiguous()
                num = eng.num_tensor(c.shape[0])
                feat = eng.pfn(example["voxels"][sel].contiguous(), c, example["num_points_per_voxel"][sel].contiguous(), num)
                rpn.append(eng.backbone(eng.scatter(feat, c, num)))
        return self.heads(torch.cat(rpn))

    def forward(self, example):
        eng = self._eng
        if example["coordinates"].dim() == 2 and example["coordinates"].shape[1] == 4:
            return self._forward_frames(example)
        voxels = example["voxels"].contiguous()
        npts = example["num_points_per_voxel"].contiguous()
        coors = example["coordinates"].contiguous()
        num = eng.num_tensor(voxels.shape[0])
        start = time.time()
        feat = eng.pfn(voxels, coors, npts, num)
        pfn_time = self._sync()
        canvas = eng.scatter(feat, coors, num)
        scatter_time = self._sync()
        rpn = eng.backbone(canvas)
        rpn_time = self._sync()
        p = self.heads(rpn)
        cls, box, dr = p["cls_preds"], p["box_preds"], p["dir_preds"]
        heads_time = self._sync()
        self.pfn_time += pfn_time - start
        self.scatter_time += scatter_time - pfn_time
        self.rpn_time += rpn_time - scatter_time
        self.heads_time += heads_time - rpn_time
        return {"cls_preds": cls, "box_preds": box, "dir_preds": dr}

    __call__ = forward

    # sub-stages, named as the reference's sub-modules, for stage-wise parity tests
    def pillar_point_net(self, voxels, num_point_per_voxel, coors):
        return self._eng.pfn(voxels.contiguous(), coors.contiguous(), num_point_per_voxel.contiguous(),
                             self._eng.num_tensor(voxels.shape[0]))[:voxels.shape[0]]

    def middle_feature_extractor(self, voxel_features, coords):
        return self._eng.scatter(voxel_features.contiguous(), coords.contiguous(), self._eng.num_tensor(coords.shape[0]))

    def rpn(self, x):
        return self._eng.backbone(x.contiguous())

    def heads(self, x):
        """SharedHead.forward on x [B,320,H,W], 1 <= B <= max_batch.  Differentiable with respect to x and the head parameters when
        one of them requires grad (train() for the parameters); gradients are fp32 and need the fp32 precision mode."""
        x = x.contiguous()
        params = list(self._params.values())
        if self._head_moved():
            self._trained = True
            self._sync_head()
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            if self._eng.effective_precision() != "fp32":
                raise RuntimeError(f"head training needs the fp32 precision mode: the network runs '{self._eng.effective_precision()}' "
                                   "(gradients are fp32 and the packed 16-bit head weights cannot be updated in place); call float()")
            if x.dim() != 4:
                x = x.reshape(-1, 320, self._eng.H, self._eng.W)
            cls, box, dr = _HeadFunction.apply(self._eng, x, *params)
        else:
            cls, box, dr = self._eng.head(x)
        return {"cls_preds": cls, "box_preds": box, "dir_preds": dr}
