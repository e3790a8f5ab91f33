"""torch reference of the CLS-row attention of a pruned last ViT layer, in the dtype of its inputs (the tests use fp64), in both forms:

  straight(...)  ln_1 of every row, K | V = rows [W, 3W) of the in-projection, one-query softmax attention per (frame, head)
  folded(...)    what acx_attention_cls_fold evaluates: u_h = W_{k,h}^T q_h, scores u_h . ln_1(x_j) / 8, z_h = sum_j p_j ln_1(x_j),
                 o_h = W_{v,h} z_h + b_{v,h}

Shared by tests/test_cpu_cls_fold.py and tests/test_gpu_cls_fold.py; not a test module itself."""
import torch

# (batch, L, W): L = 1, the tiny geometry, every backbone's token count (50 / 197 / 257 / 577), the kernel's upper limit
SHAPES = [(1, 1, 128), (3, 2, 128), (5, 50, 768), (3, 197, 768), (2, 257, 1024), (1, 577, 1024), (1, 1024, 768)]


def layer_norm(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def make_inputs(batch, L, W, seed=0, col_scale=None, q_scale=None):
    """f32 inputs of one case: x [batch * L, W] (a residual stream with a per-column offset), ln_1, the in-projection (entries of
    variance 1 / W: unit-variance q, k, v), and q = W_q ln_1(x_0) + b_q of the CLS rows, rounded to f32 like the Q launch's output.
    col_scale: column 7 of x times this (the massive-activation regime); q_scale: q times this (wide score range)."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * L + W + batch)
    x = torch.randn(batch * L, W, generator=g) * 1.3 + torch.randn(W, generator=g) * 0.4
    if col_scale is not None:
        x[:, 7] *= col_scale
    ln_w = 1.0 + 0.2 * torch.randn(W, generator=g)
    ln_b = 0.1 * torch.randn(W, generator=g)
    in_w = torch.randn(3 * W, W, generator=g) * W ** -0.5
    in_b = 0.2 * torch.randn(3 * W, generator=g)
    y0 = layer_norm(x.double().view(batch, L, W)[:, 0], ln_w.double(), ln_b.double())
    q = (y0 @ in_w[:W].double().t() + in_b[:W].double()).float()
    if q_scale is not None:
        q = q * q_scale
    return dict(x=x, ln_w=ln_w, ln_b=ln_b, in_w=in_w, in_b=in_b, q=q, batch=batch, L=L, W=W, heads=W // 64)


def _cast(c, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in c.items()}


def scores_straight(c, dtype=torch.float64, k_bias=True):
    """[batch, heads, L] q_h . k_{j,h} / 8 of the straightforward form"""
    c = _cast(c, dtype)
    B, L, W, H = c["batch"], c["L"], c["W"], c["heads"]
    y = layer_norm(c["x"], c["ln_w"], c["ln_b"]).view(B, L, W)
    k = y @ c["in_w"][W:2 * W].t()
    if k_bias:
        k = k + c["in_b"][W:2 * W]
    return torch.einsum("bhd,blhd->bhl", c["q"].view(B, H, 64), k.view(B, L, H, 64)) / 8.0


def straight(c, dtype=torch.float64, k_bias=True):
    """[batch, W]: LayerNorm, K | V projection, one-query attention"""
    s = scores_straight(c, dtype, k_bias)
    c = _cast(c, dtype)
    B, L, W, H = c["batch"], c["L"], c["W"], c["heads"]
    y = layer_norm(c["x"], c["ln_w"], c["ln_b"]).view(B, L, W)
    v = (y @ c["in_w"][2 * W:].t() + c["in_b"][2 * W:]).view(B, L, H, 64)
    return torch.einsum("bhl,blhd->bhd", torch.softmax(s, -1), v).reshape(B, W)


def folded(c, dtype=torch.float64):
    """[batch, W]: the key projection folded into the query, the value projection into the output"""
    c = _cast(c, dtype)
    B, L, W, H = c["batch"], c["L"], c["W"], c["heads"]
    y = layer_norm(c["x"], c["ln_w"], c["ln_b"]).view(B, L, W)
    wk = c["in_w"][W:2 * W].view(H, 64, W)
    wv = c["in_w"][2 * W:].view(H, 64, W)
    u = torch.einsum("bhd,hdw->bhw", c["q"].view(B, H, 64), wk)
    p = torch.softmax(torch.einsum("bhw,blw->bhl", u, y) / 8.0, -1)
    z = torch.einsum("bhl,blw->bhw", p, y)
    return (torch.einsum("hdw,bhw->bhd", wv, z) + c["in_b"][2 * W:].view(H, 64)).reshape(B, W)
