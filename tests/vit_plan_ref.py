"""The gates of the transformer driver restated on the host: what `transformer_layers` of csrc/acx_api.hip launched layer by layer at
commit e3fea90 ("Score unlabeled videos: Trainer.predict, anomaly events on the GPU"), the last commit in which the walk decided
while it launched.  Written from that file; the line numbers are its own:

    x6_takes                 227-233   the plane kernel takes a product (no planes in the workspace: never)
    linear_x6                241, 246  "missing bf16 x 3 weight planes"; a plane output of the fp16 mode is ACX_F16X2P
    linear1                  263-265   "missing %s weight copy"
    mode, dtypes             322-331   x6mode, xm, pdt3, prec -> f32, hdt, ln_ride
    cls_fold                 335-337
    the pruned last layer    340-383
    x6_qkv .. x6_proj        387-388
    ln_1                     390-395   (ln1_done: carried from the previous layer's c_proj, 455)
    ab, att_p3, att_p3f      398-404
    in-projection            405-411
    att_x3, the fp16 gate    412-414
    the attention            415-425
    split, out-proj, ln_2    426-440
    c_fc                     441-448
    split, next_planes, c_proj  449-461

`plan_ref` walks the layers as that loop did -- ln1_done carried along, a refusal returned where the walk met it -- and writes what
it would have launched in the vocabulary of acx_tf_layer_plan_t (include/acx.h).  Options: the values acx_create sets unless given.
test_cpu_vit_plan.py / test_gpu_vit_plan.py hold acx_transformer_plan against it record for record."""
from anomalyclip_amd import _lib as L

E_BADARG, E_UNSUPPORTED = -1, -2
T_PLANES = "missing bf16 x 3 weight planes"
T_COPY = "missing %s weight copy"
T_F16 = "needs the planes attention (192 < L <= 208) and all four products on the plane kernel"

FIELDS = ("ln1", "ln1_dtype", "ln2", "ln2_dtype", "in_proj", "out_proj", "fc", "proj", "att", "att_products", "split_att", "split_mlp",
          "pruned")


class Refused(Exception):
    def __init__(self, code, text):
        super().__init__(text)
        self.code, self.text = code, text


def _product(kernel, c_dtype, scratch, ln_job=0):
    return {"kernel": kernel, "c_dtype": c_dtype, "scratch": scratch, "ln_job": int(ln_job)}


def plan_ref(batch, Ltok, W, heads, layers, causal, prec, prune, has_planes, ws_prec_sized, *, x6_min_tiles=18, attn_f32in=1,
             cls_fold=1):
    """(0, [record per layer]) or (code, text fragment) of the refusal"""
    try:
        return 0, _walk(batch, Ltok, W, heads, layers, causal, prec, prune, has_planes, ws_prec_sized, x6_min_tiles, attn_f32in, cls_fold)
    except Refused as r:
        return r.code, r.text


def _walk(batch, Ltok, W, heads, layers, causal, prec, prune, has_planes, ws_prec_sized, x6_min, f32in, fold_opt):
    rows = batch * Ltok
    x6mode = prec in (L.PREC_F32X6, L.PREC_F32X3, L.PREC_F16X3)
    pairs = 3 if prec in (L.PREC_F32X3, L.PREC_F16X3) else 6
    f16 = prec == L.PREC_F16X3
    pdt3 = L.F16X2P if f16 else L.BF16X2P if prec == L.PREC_F32X3 else L.BF16X3P
    hp = x6mode and ws_prec_sized                                   # carve_tf: the planes exist in a workspace sized for the mode
    if x6mode:
        prec = L.PREC_F32
    hdt = L.ACX_BF16 if prec == L.PREC_BF16 else L.ACX_F32
    ln_ride = pdt3 == L.BF16X3P
    plane_out = L.F16X2P if f16 else L.BF16X3P                      # linear_x6: c_dtype ACX_BF16X3P of the fp16 mode

    def takes(M, N, K, lda):
        if not hp:
            return False
        rtiles = ((M + 255) // 256) * ((N + 255) // 256)
        return rtiles >= x6_min and K % 256 == 0 and N % 8 == 0 and M * lda * 2 < 2 ** 32 and N * K * 2 < 2 ** 32

    def linear():                                                   # linear1: the weight copy of the precision
        if prec == L.PREC_BF16 and not has_planes:
            raise Refused(E_BADARG, T_COPY % "bf16")

    def linear_x6():
        if not has_planes:
            raise Refused(E_BADARG, T_PLANES)

    fold_ws = rows * 3 * W * 4
    fold = bool(prune and prec != L.PREC_BF16 and fold_opt and Ltok <= 1024 and 2 * batch * heads * heads * 64 * 4 <= fold_ws)
    out = []
    ln1_done = False
    for l in range(layers):
        r = dict.fromkeys(FIELDS, 0)
        out.append(r)
        if prune and l == layers - 1:
            r["pruned"] = 1
            if fold:
                r["ln1"], r["ln1_dtype"] = L.TF_LN_CLS, hdt
                linear()
                r["in_proj"] = _product(L.TF_GEMM_ROWS, L.ACX_F32, L.TF_BUF_NONE)
                r["att"] = L.TF_ATT_CLS_FOLD
            else:
                if x6mode and takes(rows, 2 * W, W, W):
                    if not has_planes:
                        raise Refused(E_BADARG, T_PLANES)
                    r["ln1"], r["ln1_dtype"] = (L.TF_LN_RIDDEN if ln1_done else L.TF_LN_PLANES), pdt3
                    linear_x6()
                    r["in_proj"] = _product(L.TF_GEMM_X6, L.ACX_F32, L.TF_BUF_NONE)
                else:
                    r["ln1"], r["ln1_dtype"] = L.TF_LN_ROWS, hdt
                    linear()
                    r["in_proj"] = _product(L.TF_GEMM_ROWS, L.ACX_F32, L.TF_BUF_NONE)
                linear()                                            # Q
                r["att"] = L.TF_ATT_CLS
            linear()
            r["out_proj"] = _product(L.TF_GEMM_ROWS, L.ACX_F32, L.TF_BUF_NONE)
            r["ln2"], r["ln2_dtype"] = L.TF_LN_CLS, hdt
            linear()
            r["fc"] = _product(L.TF_GEMM_ROWS, hdt, L.TF_BUF_NONE)
            linear()
            r["proj"] = _product(L.TF_GEMM_ROWS, L.ACX_F32, L.TF_BUF_NONE)
            continue
        x6_qkv, x6_out = x6mode and takes(rows, 3 * W, W, W), x6mode and takes(rows, W, W, W)
        x6_fc, x6_proj = x6mode and takes(rows, 4 * W, W, W), x6mode and takes(rows, W, 4 * W, 4 * W)
        ln2_done = False
        ln1_had, ln1_done = ln1_done, False
        if x6_qkv:
            r["ln1"], r["ln1_dtype"] = (L.TF_LN_RIDDEN if ln1_had else L.TF_LN_PLANES), pdt3
        else:
            r["ln1"], r["ln1_dtype"] = L.TF_LN_ROWS, hdt
        ab = prec == L.PREC_BF16 and not causal and Ltok <= 224
        qdt = L.ACX_BF16 if ab else L.ACX_F32
        att_p3 = x6_qkv and x6_out and hp and not causal and 192 < Ltok <= 208
        att_p3f = bool(att_p3 and pdt3 == L.BF16X3P and f32in)
        qkv_planes = att_p3 and not att_p3f
        if x6_qkv:
            linear_x6()
            r["in_proj"] = (_product(L.TF_GEMM_X6, plane_out, L.TF_BUF_QKV) if qkv_planes else
                            _product(L.TF_GEMM_X6, L.ACX_F32, L.TF_BUF_H))
        else:
            linear()
            r["in_proj"] = _product(L.TF_GEMM_ROWS, qdt, L.TF_BUF_SPLITK)
        att_x3 = x6_out and not causal and 128 < Ltok <= 1024
        if f16 and (x6_qkv or x6_out or x6_fc or x6_proj) and not (att_p3 and x6_fc and x6_proj):
            raise Refused(E_UNSUPPORTED, T_F16)
        if ab:
            r["att"] = L.TF_ATT_BF16
        elif att_p3f:
            r["att"] = L.TF_ATT_P3F
        elif att_p3:
            r["att"], r["att_products"] = L.TF_ATT_P3N, (103 if f16 else pairs)
        elif att_x3:
            r["att"] = L.TF_ATT_X3_PANEL
        else:
            r["att"] = L.TF_ATT_F32
        if x6_out:
            r["split_att"] = int(not att_x3 and not att_p3)
            ln2_done = ln_ride and x6_fc
            linear_x6()
            r["out_proj"] = _product(L.TF_GEMM_X6, L.ACX_F32, L.TF_BUF_H, ln2_done)
        else:
            linear()
            r["out_proj"] = _product(L.TF_GEMM_ROWS, L.ACX_F32, L.TF_BUF_SPLITK)
        if x6_fc:
            r["ln2"], r["ln2_dtype"] = (L.TF_LN_RIDDEN if ln2_done else L.TF_LN_PLANES), pdt3
            linear_x6()
            r["fc"] = _product(L.TF_GEMM_X6, plane_out, L.TF_BUF_MLP) if x6_proj else _product(L.TF_GEMM_X6, L.ACX_F32, L.TF_BUF_H)
        else:
            r["ln2"], r["ln2_dtype"] = L.TF_LN_ROWS, hdt
            linear()
            r["fc"] = _product(L.TF_GEMM_ROWS, hdt, L.TF_BUF_SPLITK)
        if x6_proj:
            r["split_mlp"] = int(not x6_fc)
            if l + 1 < layers and prune and l + 1 == layers - 1:
                next_planes = not fold and takes(rows, 2 * W, W, W) and has_planes
            else:
                next_planes = l + 1 < layers and x6_qkv
            ln1_done = bool(ln_ride and next_planes)
            linear_x6()
            r["proj"] = _product(L.TF_GEMM_X6, L.ACX_F32, L.TF_BUF_H, ln1_done)
        else:
            linear()
            r["proj"] = _product(L.TF_GEMM_ROWS, L.ACX_F32, L.TF_BUF_SPLITK)
    return out
