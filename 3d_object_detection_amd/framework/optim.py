"""The optimizer half of the training step on the device: clip_grad_norm_ and Adam / AdamW over the library's multi-tensor HIP kernels
(csrc/optim.hip).  The reference's train.py:100-108 calls torch for both; here the two lines change only their module:

    from 3d_object_detection_amd.framework import optim          (through importlib: the package name starts with a digit)
    optimizer = optim.Adam(net.parameters(), lr=...)
    ...
    loss.backward()
    optim.clip_grad_norm_(net.parameters(), 10.0)
    optimizer.step()                      # or, fused: optimizer.step(clip_norm=10.0), which leaves the gradients as they are

The classes derive from torch.optim.Optimizer for the bookkeeping alone -- param_groups, state_dict() / load_state_dict() in torch's
layout (so checkpoints resume in both directions), zero_grad(), the hooks and the lr schedulers -- and work on CPU tensors as far as
that goes.  step() and clip_grad_norm_ run HIP kernels and need the parameters on a ROCm GPU: there is no fallback."""
import torch

__all__ = ["Adam", "AdamW", "clip_grad_norm_"]

_NO_GPU = "3d_object_detection_amd needs a ROCm GPU: the HIP path has no CPU fallback"


def _engine(tensors):
    """The kernels need a context only for the device and for error text: a live engine on the tensors' device
    (framework/augmentation.py:_engine)."""
    if not torch.cuda.is_available() or not all(t.is_cuda for t in tensors):
        raise RuntimeError(_NO_GPU + " (the optimizer's parameters and gradients must be on the GPU)")
    from .augmentation import _engine as live_engine
    return live_engine(tensors[0].device)


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False):
    """torch.nn.utils.clip_grad_norm_ for the 2-norm: scales the gradients in place by min(1, max_norm / (total_norm + 1e-6)) and
    returns the total norm as a 0-dim float32 tensor on the device.  The norm is summed in fp64 in a fixed order (two runs agree bit for
    bit) and nothing synchronises with the host unless error_if_nonfinite is set."""
    if float(norm_type) != 2.0:
        raise NotImplementedError(f"clip_grad_norm_: only norm_type 2 runs on the device, got {norm_type}")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    eng = _engine(grads)
    out = eng.grad_norm(grads, max_norm)
    if error_if_nonfinite and not bool(torch.isfinite(out[0])):
        raise RuntimeError(f"The total norm of order {float(norm_type)} for gradients from `parameters` is non-finite, so it cannot be "
                           "clipped. To disable this error and scale the gradients by the non-finite norm anyway, set "
                           "`error_if_nonfinite=False`")
    eng.scale_grads(grads, out[1:])
    torch.autograd.graph.increment_version(grads)
    return out[0]


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam with one parameter group, stepped by pp_adam_step.  Hyper-parameters are read from param_groups[0] at every
    step, so assigning param_groups[0]['lr'] (train.py:73, the lr schedulers) takes effect; the keys are the ones torch writes."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 decoupled_weight_decay=False):
        if amsgrad or maximize:
            raise NotImplementedError("the device optimizer runs plain Adam / AdamW: amsgrad and maximize are not implemented")
        if isinstance(params, torch.Tensor):
            raise TypeError("params must be an iterable of tensors, not one tensor")
        params = list(params)
        if any(isinstance(p, dict) for p in params):
            raise NotImplementedError("the device optimizer takes one parameter group: pass the tensors, not a list of dicts")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # the keys, order and values of torch.optim.Adam's defaults: a state_dict() written here is one of torch's
        defaults = {"lr": lr, "betas": tuple(float(b) for b in betas), "eps": eps, "weight_decay": weight_decay, "amsgrad": False,
                    "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                    "decoupled_weight_decay": decoupled_weight_decay}
        super().__init__(params, defaults)

    @torch.no_grad()
    def step(self, closure=None, clip_norm=None):
        """One step over the parameters that have a gradient; the others keep their value, their state and their step count.
        clip_norm: the fused form of clip_grad_norm_(params, clip_norm) followed by step() -- the same bits in the parameters and
        moments, with the gradients left untouched; returns the total norm (0-dim device tensor).  Otherwise returns the closure's
        loss, as torch does.  Every tensor is checked before the first kernel is launched."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if len(self.param_groups) != 1:
            raise NotImplementedError("the device optimizer takes one parameter group")
        group = self.param_groups[0]
        if group.get("amsgrad") or group.get("maximize"):
            raise NotImplementedError("the device optimizer runs plain Adam / AdamW: amsgrad and maximize are not implemented")
        every = group["params"]
        idx = [i for i, p in enumerate(every) if p.grad is not None]
        if not idx:
            return torch.tensor(0.0) if clip_norm is not None else loss
        params = [every[i] for i in idx]
        grads = [p.grad for p in params]
        if any(g.is_sparse for g in grads):
            raise RuntimeError("Adam does not support sparse gradients")
        eng = _engine(params + grads)
        plan = self._plan_for(eng, every, idx, params)
        pg = eng._chk_list(grads, "Adam.step: grads", like=params)
        steps = plan["steps"].tolist()
        ts = sorted({int(steps[i]) + 1 for i in idx})
        beta1, beta2 = group["betas"]
        hyper = (float(group["lr"]), float(beta1), float(beta2), float(group["eps"]), float(group["weight_decay"]),
                 int(bool(group.get("decoupled_weight_decay", False))))
        out = eng._grad_norm(pg, plan["lens"], len(params), float(clip_norm)) if clip_norm is not None else None
        coef = None if out is None else out[1:]
        if len(ts) == 1:
            eng._adam_step(plan["p"], pg, plan["m"], plan["v"], plan["lens"], len(params), ts[0], *hyper, coef)
        else:  # parameters that sat out a step lag behind the others: one call per distinct step number
            for t in ts:
                sel = [k for k, i in enumerate(idx) if int(steps[i]) + 1 == t]
                eng.adam_step([params[k] for k in sel], [grads[k] for k in sel], [plan["state"][k]["exp_avg"] for k in sel],
                              [plan["state"][k]["exp_avg_sq"] for k in sel], t, *hyper[:5], decoupled=hyper[5], coef=coef)
        if plan["sel"] is None:
            plan["steps"] += 1
        else:
            plan["steps"][plan["sel"]] += 1
        for p, st in zip(params, plan["state"]):  # state appears once the step it belongs to has run
            if self.state.get(p) is not st:
                self.state[p] = st
        # the kernels wrote through raw pointers: move the version counters so that whatever caches derived data (the network's
        # packed weight images) sees the step, as it does after a torch optimizer
        torch.autograd.graph.increment_version(params)
        return out[0] if out is not None else loss

    def _plan_for(self, eng, every, idx, params):
        """What a step needs of the tensors the optimizer owns, kept between steps: the state dicts of the stepped parameters, the
        host arrays of their p / exp_avg / exp_avg_sq pointers and lengths, and the step counts -- state[p]['step'] of all
        parameters are 0-dim views of ONE float32 CPU tensor, so that reading and advancing 28 counters is one operation each.  Kept
        while the same parameter objects at the same addresses carry the same state objects; rebuilt (state created where missing, as
        torch creates it; everything checked; counters gathered from whatever load_state_dict or the user put there) otherwise."""
        plan = getattr(self, "_plan", None)
        if plan is not None and plan["idx"] == idx and len(plan["every"]) == len(every) and all(a is b for a, b in zip(plan["every"], every)):
            get = self.state.get
            for p, ptr, st, m, v, s in zip(params, plan["ptr"], plan["state"], plan["mt"], plan["vt"], plan["st"]):
                cur = get(p)
                if p.data_ptr() != ptr or (cur is not st and cur) or st["exp_avg"] is not m or st["exp_avg_sq"] is not v or st["step"] is not s:
                    break
            else:
                return plan
        steps = torch.zeros(len(every), dtype=torch.float32)
        for i, p in enumerate(every):
            st = self.state.get(p)
            if st:
                steps[i] = float(st["step"])
                st["step"] = steps[i]
        state = []
        for i, p in zip(idx, params):
            st = self.state.get(p)
            if not st:  # not self.state[p]: a refused step leaves no entry behind
                st = {"step": steps[i], "exp_avg": torch.zeros_like(p, memory_format=torch.preserve_format),
                      "exp_avg_sq": torch.zeros_like(p, memory_format=torch.preserve_format)}
            state.append(st)
        mt, vt = [st["exp_avg"] for st in state], [st["exp_avg_sq"] for st in state]
        plan = {"idx": idx, "every": list(every), "state": state, "mt": mt, "vt": vt, "st": [st["step"] for st in state],
                "p": eng._chk_list(params, "Adam.step: params"), "m": eng._chk_list(mt, "Adam.step: exp_avg", like=params),
                "v": eng._chk_list(vt, "Adam.step: exp_avg_sq", like=params), "lens": eng._lens(params),
                "ptr": [p.data_ptr() for p in params], "steps": steps,
                "sel": None if len(idx) == len(every) else torch.tensor(idx, dtype=torch.int64)}
        self._plan = plan
        return plan


class AdamW(Adam):
    """torch.optim.AdamW: Adam with decoupled weight decay (p -= lr weight_decay p before the moment update)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize, decoupled_weight_decay=True)
