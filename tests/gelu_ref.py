"""The exact GELU in fp64 and the yardstick the device function is held to (tests/test_gpu_gelu*.py, tests/test_cpu_gelu.py): plain
torch, importable without a GPU.  (In tests/gemm_ref.py `GELU` means QuickGELU; here it means nn.GELU, 0.5 x (1 + erf(x / sqrt 2)).)

sweep() is the input set of the function tests: torch.linspace(-12, 12, 2_000_001), 1e6 draws of 3 randn and the edge values.
yardstick() measures torch's OWN float32 CPU F.gelu against fp64 on that sweep -- forward as max |err| / max(|x|, 1), derivative
(autograd) as max |err| -- and the device function may have at most MARGIN = 2 times that: a device erf one or two ulp looser than
libm's fits, an approximation of another kind (tanh form: ~5e-4) does not."""
import functools
import math

import torch
import torch.nn.functional as F

MARGIN = 2.0
EDGES = [0.0, -0.0, 1e-30, -1e-30, 1e-5, -1e-5, 6.0, -6.0, 9.0, -9.0, 30.0, -30.0, 1e4, -1e4]


def gelu64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu64_grad(x):
    x = x.double()
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def quick_gelu64(x):
    x = x.double()
    return x * torch.sigmoid(1.702 * x)


@functools.lru_cache(maxsize=None)
def sweep():
    g = torch.Generator().manual_seed(20240)
    return torch.cat([torch.linspace(-12, 12, 2_000_001), 3.0 * torch.randn(1_000_000, generator=g), torch.tensor(EDGES)]).float()


def fwd_scale(x):
    return x.double().abs().clamp_min(1.0)


@functools.lru_cache(maxsize=None)
def yardstick():
    """(forward, derivative): the fp64 error of torch's float32 CPU F.gelu on sweep(), forward relative to max(|x|, 1), derivative
    absolute -- both computed here, never hard-coded"""
    x = sweep()
    with torch.enable_grad():                              # (whatever a module imported earlier left the global switch at)
        x64 = x.double().requires_grad_(True)
        r = F.gelu(x64)
        (g64,) = torch.autograd.grad(r.sum(), x64)
        x32 = x.clone().requires_grad_(True)
        y = F.gelu(x32)
        (g32,) = torch.autograd.grad(y.sum(), x32)
    fwd = ((y.detach().double() - r.detach()).abs() / fwd_scale(x)).max().item()
    grad = (g32.double() - g64).abs().max().item()
    return fwd, grad


def fwd_term(pre):
    """the function-error term of a GELU epilogue at fp64 pre-activation `pre`: MARGIN x yardstick x max(|pre|, 1)"""
    return MARGIN * yardstick()[0] * fwd_scale(pre)


def grad_term():
    return MARGIN * yardstick()[1]
