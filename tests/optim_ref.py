"""Float64 restatement of what the device optimizer computes (csrc/optim.hip, framework/optim.py): the clip coefficient of
torch.nn.utils.clip_grad_norm_ and one Adam / Adam-with-L2 / AdamW step from a given (p, g, m, v, t) -- pinned to torch's own float64
run by test_optim_cpu.py -- and the seeded tensor lists the CPU and GPU tests share."""
import numpy as np

F64 = np.float64


def total_norm(grads):
    return float(np.sqrt(sum(float((np.asarray(g, F64) ** 2).sum()) for g in grads if g is not None)))


def clip_coef(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6)); a NaN norm gives NaN (torch.clamp(nan, max=1) is nan)."""
    c = max_norm / (norm + 1e-6)
    return c if not c > 1.0 else 1.0


def adam_step(p, g, m, v, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=False, coef=1.0):
    """One step at step number t >= 1 -> (p, m, v) in float64.  The inputs are not changed."""
    p, g, m, v = (np.array(x, F64) for x in (p, g, m, v))
    g = coef * g
    if weight_decay != 0 and not decoupled:
        g = g + weight_decay * p
    if weight_decay != 0 and decoupled:
        p = p - lr * weight_decay * p
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    p = p - (lr / (1 - beta1 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - beta2 ** t) + eps)
    return p, m, v


def values(rng, n):
    """p ~ 0.05 N(0,1), g ~ 1e-2 N(0,1) with every 7th element exactly 0, m ~ 3e-3 N(0,1), v = (1e-2 N(0,1))^2, float32."""
    p = (0.05 * rng.standard_normal(n)).astype(np.float32)
    g = (1e-2 * rng.standard_normal(n)).astype(np.float32)
    g[::7] = 0
    m = (3e-3 * rng.standard_normal(n)).astype(np.float32)
    v = ((1e-2 * rng.standard_normal(n)) ** 2).astype(np.float32)
    return dict(p=p, g=g, m=m, v=v)


def main_list(chunk, seed=0):
    """The chunk-edge sizes, one tensor to be placed one element into a larger buffer ("view": 4-byte aligned only; a whole chunk and
    a tail), one empty tensor and one parameter without a gradient (g None)."""
    rng = np.random.default_rng(seed)
    out = []
    for n in (1, 3, 4, 5, 63, 576, chunk - 1, chunk, chunk + 1, 2 * chunk + 7):
        out.append(dict(values(rng, n), kind="plain"))
    out.append(dict(values(rng, chunk + 5), kind="view"))
    out.append(dict(values(rng, 0), kind="empty"))
    out.append(dict(values(rng, 10), kind="nograd"))
    out[-1]["g"] = None
    return out


def many_list(seed=1, count=70, n=5):
    """More tensors than one launch takes."""
    rng = np.random.default_rng(seed)
    return [dict(values(rng, n), kind="plain") for _ in range(count)]
