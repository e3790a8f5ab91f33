"""numpy fp64 restatement of gradient clipping followed by AdamW -- what torch.nn.utils.clip_grad_norm_ / clip_grad_value_ and
torch.optim.AdamW compute, written out so that the tests have a reference that shares no code with the library:

  norm         sqrt of the fp64 sum of squares of the F32-ROUNDED g * scale (the square of an f32 is exact in fp64)
  coefficient  torch's, in f32: c = max_norm / (norm + 1e-6), then c > 1 ? 1 : c  (a NaN stays a NaN)
  clipping     "norm": (g * scale) * c in f32;  "value": g * scale clamped to [-v, v], NaN kept
  AdamW        decoupled weight decay, bias correction, no amsgrad, in fp64"""
import numpy as np

F32 = np.float32


def scaled(g, scale=1.0):
    return (np.asarray(g, dtype=F32) * F32(scale)).astype(F32)


def grad_norm(grads, scale=1.0) -> float:
    """fp64 global L2 norm of the f32 values g * scale"""
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.sqrt(sum(float(np.sum(scaled(g, scale).astype(np.float64) ** 2)) for g in grads)))


def clip_coef(norm, max_norm) -> np.float32:
    """the f32 coefficient torch forms from an f32 norm"""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        c = F32(max_norm) / (F32(norm) + F32(1e-6))
    return F32(1.0) if c > F32(1.0) else c


def clip(grads, algorithm, value, scale=1.0):
    """-> (clipped f32 gradients, f32 norm or None)"""
    if algorithm == "value":
        out = []
        for g in grads:
            x = scaled(g, scale)
            out.append(np.where(x > F32(value), F32(value), np.where(x < -F32(value), -F32(value), x)).astype(F32))
        return out, None
    assert algorithm == "norm"
    with np.errstate(over="ignore", invalid="ignore"):
        norm = F32(grad_norm(grads, scale))
        c = clip_coef(norm, value)
        return [(scaled(g, scale) * c).astype(F32) for g in grads], norm


def adamw_step(p, g, m, v, lr, weight_decay, beta1, beta2, eps, step):
    """one torch.optim.AdamW step in fp64 -> (p, m, v)"""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    p = p * (1.0 - lr * weight_decay)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    p = p - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
    return p, m, v
