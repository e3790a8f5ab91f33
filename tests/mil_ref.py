"""Test infrastructure for the selector / MIL chain (select_idx -> gather_segments -> mil_loss / mil_loss_bn -> scatter_segments_ ->
bn_bwd_stats -> bn_bwd_apply -> gemm_tn -> text_directions_bwd): the fp64 closed forms of the loss with its three gradients, of the
training BatchNorm backward and of the direction normalisation backward, each with the term magnitude S its error is judged
against, and the seeded inputs of the sweeps.  CPU only; nothing here touches the GPU side.  The method is rowwise_ref's:

    |err| <= TOL * S   element by element, TOL = 2e-6, S = the sum of the absolute values of the terms the element is made of,
    and an element with S == 0 is exact.

Where TOL comes from: torch's own fp32 CPU evaluation of oracle.compute_loss / a plain BatchNorm expression /
oracle.selector_directions with autograd, on the inputs below, against these closed forms (tests/test_cpu_mil_ref.py repeats the
measurement and asserts half the bound); the worst |err| / S it shows are recorded in DESIGN.md section 3.  The bound is never set
from what the kernels give.

The inputs are the hard ones: sim = 6 randn (peaked softmax rows: p_y down to e^-40), a tenth of the scores within 1e-4 of 0 and a
tenth within 1e-4 of 1 (1 / sc and 1 / (1 - sc) up to 1e6), abnormal labels on both sides of normal_id, seven distinct lambdas (a
permutation of them changes every term), and BatchNorm columns whose mean is up to 500 standard deviations away from 0."""
import torch

from oracle import anomalyclip_oracle as O

TOL = 2e-6
LAMBDAS = (0.7, 1.3, 0.9, 1.7, 0.6, 3e-3, 5e-2)       # dir_abn, dir_nor, topk_abn, bottomk_abn, topk_nor, smooth, sparse
GOUT = 2.5
LOSS_NAMES = ("cost", "ldir_abn", "ldir_nor", "ltopk_abn", "lbottomk_abn", "ltopk_nor", "lsmooth", "lsparse")

# (B, N, Lg, C1, K, normal_id)
LOSS_SWEEP = [
    (2, 5, 7, 1, 1, 0),          # C1 = 1: softmax == 1, dsim == 0 on the top-k rows; 70 rows: one ragged block
    (4, 24, 10, 6, 2, 3),        # 960 rows: a ragged last block of four
    (6, 7, 5, 13, 3, 13),        # normal_id is the last class (no label shifts), odd B / 2
    (8, 32, 16, 13, 3, 7),       # the workload grid; B K Lg = 384: two top-k blocks
    (4, 3, 4, 64, 3, 20),        # C1 = 64 (the limit), K = N
    (2, 40, 12, 16, 5, 0),       # normal_id = 0 (every label shifts), K = 5
    (16, 64, 16, 17, 3, 8),      # 64 row blocks
    (64, 32, 16, 13, 3, 7),      # 128 row blocks: four parts per lane in the last arriver's strided sum, 12 top-k blocks
]
LOSS_BN_EXTRA = [(2, 8, 16, 1, 1, 0), (4, 16, 32, 64, 3, 20)]      # B N Lg % 256 == 0 at C1 = 1 and C1 = 64
BN_SWEEP = [(70, 1), (960, 6), (257, 64), (4099, 40), (131072 + 259, 13)]      # (rows, C1); the last: more than 512 slabs' worth
DIRS_SWEEP = [(2, 64, 0), (2, 64, 1), (14, 512, 7), (7, 768, 6), (18, 1024, 4), (65, 256, 20), (9, 640, 0), (5, 2560, 2)]


def case_id(case):
    return "-".join(str(int(v)) for v in case)


# ------------------------------------------------------------------------------------------------------------- the step graph's gates
# The shapes the one-launch forms take, as the training step evaluated them itself before the library answered
# (acx_selector_tail_fits / acx_mil_loss_bn_fits); frozen here, tests/test_cpu_mil_ref.py holds the queries to them.
def selector_tail_gate(B, N, Lg, C1, ktop, kbot):
    """a video's logits, segment sums, keys, statistics and picks within 160 KB of LDS, at most 64 directions"""
    return (N * Lg * C1 + N * C1 + 2 * N + 2 * C1 + ktop + kbot) * 4 <= 160 * 1024 and C1 <= 64


def mil_loss_bn_gate(B, N, Lg, C1, K):
    """whole slabs of 256 frame rows, at most 512 of them, at most 64 directions"""
    rows = B * N * Lg
    return rows % 256 == 0 and rows <= 131072 and C1 <= 64


# ------------------------------------------------------------------------------------------------------------- inputs
def abnormal_labels(nv, C1, normal_id):
    """nv labels out of {0..C1} \\ {normal_id}: normal_id + 1, the largest class, normal_id - 1, the smallest, then the rest, in
    that order of preference (so both sides of normal_id appear as soon as nv >= 3 and the class list has both)"""
    classes = [c for c in range(C1 + 1) if c != normal_id]
    pref = [c for c in (normal_id + 1, classes[-1], normal_id - 1, classes[0]) if c in classes]
    order = list(dict.fromkeys(pref + classes))
    return torch.tensor([order[i % len(order)] for i in range(nv)], dtype=torch.int64)


def hard_scores(n, g):
    """a tenth within 1e-4 of 0, a tenth within 1e-4 of 1, the rest uniform; clamped to [1e-6, 1 - 1e-6]"""
    sc = torch.rand(n, generator=g)
    kind = torch.rand(n, generator=g)
    edge = torch.rand(n, generator=g) * 1e-4
    sc = torch.where(kind < 0.1, edge, torch.where(kind > 0.9, 1 - edge, sc))
    return sc.clamp(1e-6, 1 - 1e-6)


def loss_inputs(case, seed=None):
    """sim [B N Lg, C1] = 6 randn (continuous: no argmax ties), labels (abnormal half first), scores, the three index tensors
    (K distinct segments per video), sim_topk gathered from sim by (idx_topk_abn | idx_topk_nor) -- f32 / int64 CPU tensors"""
    B, N, Lg, C1, K, normal_id = case
    g = torch.Generator().manual_seed(1000 + sum((i + 1) * v for i, v in enumerate(case)) if seed is None else seed)
    rows = B * N * Lg
    sim = 6 * torch.randn(rows, C1, generator=g)
    scores = hard_scores(rows, g)
    labels = torch.cat([abnormal_labels(B // 2, C1, normal_id), torch.full((B - B // 2,), normal_id, dtype=torch.int64)])
    pick = lambda: torch.stack([torch.randperm(N, generator=g)[:K] for _ in range(B // 2)])          # noqa: E731
    ia, in_, ba = pick(), pick(), pick()
    sim_topk = O.gather_segments(sim.view(B, N * Lg, C1), torch.cat([ia, in_]), N, Lg).contiguous()
    return dict(sim=sim, sim_topk=sim_topk, labels=labels, scores=scores, idx_topk_abn=ia, idx_topk_nor=in_, idx_bottomk_abn=ba)


def bn_inputs(rows, C1, seed):
    """raw [rows, C1]: column c has mean 50 (-1)^c c / C1 and a standard deviation between 0.1 and 3 (E[x^2] - mean^2 cancels up to
    2.5e5-fold); dl [rows, C1] with a per-column scale"""
    g = torch.Generator().manual_seed(seed)
    c = torch.arange(C1, dtype=torch.float32)
    mean = 50 * (-1) ** c * c / C1
    sd = 0.1 * 30 ** (((7 * c) % C1) / max(C1 - 1, 1)) if C1 > 1 else torch.tensor([0.1])
    raw = torch.randn(rows, C1, generator=g) * sd + mean
    dl = torch.randn(rows, C1, generator=g) * torch.exp2(torch.randint(-4, 5, (1, C1), generator=g).float())
    return raw, dl


def dirs_inputs(Cc, D, seed):
    """text [C, D], ncentroid [D], ddirs [C - 1, D] with a per-row scale"""
    g = torch.Generator().manual_seed(seed)
    text = torch.randn(Cc, D, generator=g) * 0.5 + 0.1
    nc = torch.randn(D, generator=g) * 0.3
    dd = torch.randn(Cc - 1, D, generator=g) * torch.exp2(torch.randint(-4, 5, (Cc - 1, 1), generator=g).float())
    return text, nc, dd


def select_inputs(B, N, Lg, C1, normal_id, ktop, kbot, seed, shift=0):
    """logits [B, N Lg, C1] in multiples of 2^-6 within [-4, 4] (every segment sum and class sum is exact in fp32 in any order),
    labels, and two DIFFERENT masks: the row kinds (all zero, one survivor, exactly k survivors, full) go round the videos, the
    top mask starting at kind `shift`, the bottom mask one kind further; videos past the fourth draw 70 % survivors.  Every video has
    a duplicated segment: segment a's logits copied onto segment b > a, both surviving one of the masks where two survive -- exact
    ties away from the +-1e6 fill, in the abnormal and in the normal half."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randint(-256, 257, (B, N, Lg, C1), generator=g).float() / 64
    labels = torch.cat([abnormal_labels(B // 2, C1, normal_id), torch.full((B - B // 2,), normal_id, dtype=torch.int64)])

    def mask(k, first):
        m = (torch.rand(B, N, generator=g) < 0.7).float()
        for v in range(min(B, 4)):
            keep = (0, 1, min(k, N), N)[(v + first) % 4]
            m[v] = 0
            m[v, torch.randperm(N, generator=g)[:keep]] = 1
        return m
    mt, mb = mask(ktop, shift), mask(kbot, shift + 1)
    if N >= 2:
        for v in range(B):
            alive = max((mt[v].nonzero().view(-1), mb[v].nonzero().view(-1)), key=len)
            if len(alive) < 2:
                alive = torch.arange(N)
            a, b = sorted(alive[torch.randperm(len(alive), generator=g)[:2]].tolist())
            logits[v, b] = logits[v, a]
    return logits.view(B, N * Lg, C1).contiguous(), labels, mt, mb


def segment_rows(idx, N, Lg):
    """the frame rows of logits [B N Lg, .] that the rows of gather_segments(., idx) come from: ((v N + idx[v, k]) Lg + l)"""
    B, K = idx.shape
    seg = torch.arange(B).view(B, 1) * N + idx
    return (seg.view(B, K, 1) * Lg + torch.arange(Lg)).reshape(-1)


# ------------------------------------------------------------------------------------------------------------- loss
def mil_loss(sim, sim_topk, labels, scores, idx_topk_abn, idx_topk_nor, idx_bottomk_abn, N, Lg, K, normal_id, lambdas, gout=1.0):
    """{"losses", "dsim", "dsim_topk", "dscores"} -> (value, S) in fp64; losses in LOSS_NAMES order, the gradients those of gout * cost.

    With Bh = B / 2 abnormal and Bn = B - Bh normal videos, RA = Bh K Lg, y = the video's own direction, p = softmax(sim row):
      ldir_abn = -l0 mean_{RA top-k rows} sim_topk[., y]      ldir_nor = l1 mean_{normal rows} max_c sim
      ltopk_abn = l2 mean_{abn top-k} -log(p_y sc)            lbottomk_abn = l3 mean_{abn bottom-k} -log(1 - sc)
      ltopk_nor = l4 mean_{nor top-k} -log(1 - sc)            lsmooth = l5 sum (sc[r+1] - sc[r])^2 over the FLATTENED abnormal scores
      lsparse = l6 mean_{abnormal rows} sc                    S of a term: lambda * mean |summand|; S of the cost: the sum of the seven
      dsim, abnormal top-k rows:  w2 (p_c - [c = y]),  w2 = l2 gout / RA            S: w2 (p_c (1 + max_c' s_c' - s_c) + [c = y])
        (p_c = exp(s_c - max) / sum: the exponent's rounding is 2^-24 (max - s_c) relative to p_c)
      dsim, normal rows:  l1 gout / (Bn N Lg) at the argmax column                    S: the same;  S = 0 (exact zero) everywhere else
      dsim_topk:  -l0 gout / RA at column y of the RA abnormal rows                  S: the same;  S = 0 elsewhere
      dscores:  -w2 / sc [abn top-k]  +  w3 / (1 - sc) [abn bottom-k]  +  w4 / (1 - sc) [nor top-k]
                +  l5 gout 2 ((sc[r] - sc[r-1]) - (sc[r+1] - sc[r]))  +  l6 gout / Ta   [abnormal rows, Ta = Bh N Lg]
                S: w2 / sc + w3 / (1 - sc) + w4 / (1 - sc) + l5 gout 2 (|sc[r+1] - sc[r]| + |sc[r] - sc[r-1]|) + l6 gout / Ta"""
    f = torch.float64
    sim, sim_topk, sc = sim.to(f), sim_topk.to(f), scores.to(f)
    l0, l1, l2, l3, l4, l5, l6 = (float(x) for x in lambdas)
    gout = float(gout)
    R, C1 = sim.shape
    B = labels.shape[0]
    Bh, Bn, per = B // 2, B - B // 2, N * Lg
    Ta, RA = Bh * per, Bh * K * Lg
    y = torch.where(labels[:Bh] > normal_id, labels[:Bh] - 1, labels[:Bh])

    def rows_of(idx):                                   # [videos, K] segment picks -> bool [videos * per]
        m = torch.zeros(idx.shape[0], N, dtype=torch.bool).scatter_(1, idx, True)
        return m.view(-1, N, 1).expand(-1, -1, Lg).reshape(-1)
    top_a, bot_a, top_n = rows_of(idx_topk_abn), rows_of(idx_bottomk_abn), rows_of(idx_topk_nor)

    sa, sca, scn = sim[:Ta], sc[:Ta], sc[Ta:]
    yr = y.view(-1, 1).expand(-1, per).reshape(-1, 1)                                   # own direction of every abnormal row
    mx = sa.max(-1, keepdim=True)[0]
    lse = torch.logsumexp(sa, -1, keepdim=True)
    p = torch.exp(sa - lse)
    onehot = torch.zeros_like(sa).scatter_(1, yr, 1.0)
    t_top = -((sa.gather(1, yr) - lse).view(-1) + torch.log(sca))                       # -log(p_y sc)
    own = sim_topk[:RA].gather(1, y.view(-1, 1).expand(-1, K * Lg).reshape(-1, 1)).view(-1)
    nmax, nam = sim[Ta:].max(-1)
    d = sca[1:] - sca[:-1]

    terms = [(-l0 * own.mean(), l0 * own.abs().mean()),
             (l1 * nmax.mean(), l1 * nmax.abs().mean()),
             (l2 * t_top[top_a].sum() / RA, l2 * t_top[top_a].abs().sum() / RA),
             (l3 * -torch.log(1 - sca[bot_a]).sum() / RA, l3 * torch.log(1 - sca[bot_a]).abs().sum() / RA),
             (l4 * -torch.log(1 - scn[top_n]).sum() / (Bn * K * Lg), l4 * torch.log(1 - scn[top_n]).abs().sum() / (Bn * K * Lg)),
             (l5 * (d * d).sum(), l5 * (d * d).sum()),
             (l6 * sca.mean(), l6 * sca.abs().mean())]
    losses = torch.stack([sum(t[0] for t in terms)] + [t[0] for t in terms])
    s_losses = torch.stack([sum(t[1] for t in terms)] + [t[1] for t in terms])

    w2, w3, w4 = l2 * gout / RA, l3 * gout / RA, l4 * gout / (Bn * K * Lg)
    dsim, s_dsim = torch.zeros_like(sim), torch.zeros_like(sim)
    ta = top_a.view(-1, 1).to(f)
    dsim[:Ta] = ta * w2 * (p - onehot)
    s_dsim[:Ta] = ta * w2 * (p * (1 + mx - sa) + onehot)
    wn = l1 * gout / (Bn * per)
    dsim[Ta:].scatter_(1, nam.view(-1, 1), wn)
    s_dsim[Ta:].scatter_(1, nam.view(-1, 1), abs(wn))

    dtopk = torch.zeros_like(sim_topk)
    dtopk[:RA].scatter_(1, y.view(-1, 1).expand(-1, K * Lg).reshape(-1, 1), -l0 * gout / RA)

    dl, dr = torch.zeros(Ta, dtype=f), torch.zeros(Ta, dtype=f)                         # sc[r] - sc[r-1], sc[r+1] - sc[r]
    dl[1:], dr[:-1] = d, d
    ta, ba, tn = top_a.to(f), bot_a.to(f), top_n.to(f)
    dsc, s_dsc = torch.zeros(R, dtype=f), torch.zeros(R, dtype=f)
    dsc[:Ta] = -ta * w2 / sca + ba * w3 / (1 - sca) + l5 * gout * 2 * (dl - dr) + l6 * gout / Ta
    s_dsc[:Ta] = ta * w2 / sca + ba * w3 / (1 - sca) + l5 * gout * 2 * (dl.abs() + dr.abs()) + l6 * gout / Ta
    dsc[Ta:] = tn * w4 / (1 - scn)
    s_dsc[Ta:] = tn * w4 / (1 - scn)
    return {"losses": (losses, s_losses), "dsim": (dsim, s_dsim), "dsim_topk": (dtopk, dtopk.abs()), "dscores": (dsc, s_dsc)}


def dlogits(ref, idx_topk, N, Lg):
    """(dsim + scatter(dsim_topk), S) of a mil_loss result: what mil_loss_bn returns as dlogits; idx_topk = (abn | nor) [B, K]"""
    rows = segment_rows(idx_topk, N, Lg)
    return (ref["dsim"][0].index_add(0, rows, ref["dsim_topk"][0]), ref["dsim"][1].index_add(0, rows, ref["dsim_topk"][1]))


# ------------------------------------------------------------------------------------------------------------- BatchNorm / directions
def bn_col_sums(logits, dl):
    """((sum dl, sum dl xhat) [2 C1], (sum |dl|, sum |dl xhat|)) in fp64: acx_bn_bwd_stats"""
    x, g = logits.double(), dl.double()
    return torch.cat([g.sum(0), (g * x).sum(0)]), torch.cat([g.abs().sum(0), (g * x).abs().sum(0)])


def bn_bwd(logits, dl, var_b, n, eps=1e-5, sums=None):
    """(draw, S) of the training BatchNorm backward from the normalised logits xhat AS GIVEN and the biased variance:
    draw = rstd (dl - sum dl / n - xhat sum(dl xhat) / n)      S = rstd (|dl| + sum|dl| / n + |xhat| sum|dl xhat| / n)
    sums [2 C1] (sum dl | sum dl xhat): taken as given where the kernel is handed them; S keeps the sums of absolute values"""
    x, g = logits.double(), dl.double()
    rstd = 1.0 / torch.sqrt(var_b.double() + eps)
    C1 = logits.shape[1]
    s, a = bn_col_sums(logits, dl)
    if sums is not None:
        s = sums.double()
    return (rstd * (g - s[:C1] / n - x * s[C1:] / n), rstd * (g.abs() + a[:C1] / n + x.abs() * a[C1:] / n))


def dirs_fwd(text, nc, normal_id):
    """(dirs, S): v = text[src] - nc, dirs = v / |v|, S = (|t| + |nc|) / |v|"""
    t = torch.cat((text[:normal_id], text[normal_id + 1:])).double()
    v = t - nc.double()
    nrm = v.norm(dim=-1, keepdim=True)
    return v / nrm, (t.abs() + nc.double().abs()) / nrm


def dirs_bwd(text, nc, ddirs, normal_id):
    """(dtext [C, D], S): dtext[src] = (dd - v (v . dd) / |v|^2) / |v|, S = (|dd| + |v| sum|v dd| / |v|^2) / |v|; row normal_id: 0, S 0"""
    Cc = text.shape[0]
    keep = [c for c in range(Cc) if c != normal_id]
    v = text.double()[keep] - nc.double()
    dd = ddirs.double()
    n2 = (v * v).sum(-1, keepdim=True)
    nrm = n2.sqrt()
    out, S = torch.zeros(text.shape, dtype=torch.float64), torch.zeros(text.shape, dtype=torch.float64)
    out[keep] = (dd - v * (v * dd).sum(-1, keepdim=True) / n2) / nrm
    S[keep] = (dd.abs() + v.abs() * (v * dd).abs().sum(-1, keepdim=True) / n2) / nrm
    return out, S


# ------------------------------------------------------------------------------------------------------------- comparison
def ratio(out, ref, S):
    """worst |out - ref| / S over the elements with S > 0 (an element with S == 0 must be exact: reported as inf otherwise)"""
    err = (torch.as_tensor(out).detach().double().cpu() - ref.double()).abs()
    S = S.double().expand_as(err)
    r = torch.where(S > 0, err / S.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


def within(out, ref, S, what="", family=None, tol=TOL):
    """|out - ref| <= tol * S element by element; prints the worst ratio first (family: the tag the recorded ratios are grouped by)"""
    out = torch.as_tensor(out)
    r = ratio(out, ref, S)
    if family:
        print(f"MIL_RATIO {family} {what} {r:.3e}")
    return out.shape == ref.shape and bool(torch.isfinite(out).all()) and r <= tol
