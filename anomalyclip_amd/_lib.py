"""ctypes binding of libacx (include/acx.h).  The library is the product's only compute path: if it
cannot be loaded the package raises, it never falls back to PyTorch ops or to the oracle."""
from __future__ import annotations

import ctypes as C
import os
import threading

from . import _build

c_void_p, c_int32, c_int64, c_float, c_size_t = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t

ACX_F32, ACX_BF16, BF16X3, BF16X3P = 0, 1, 2, 3      # BF16X3 / BF16X3P: output only (three bf16 planes hi | mid | lo; P: K-panel layout)
BF16X2P, ACX_F16, F16X2P = 4, 5, 6                     # hi + mid planes only; fp16 planes of the two-plane split (pairs = 3); their K-panel output
PREC_F32, PREC_BF16, PREC_F32X6, PREC_F32X3, PREC_F16X3 = 0, 1, 2, 3, 4
PREC_BF16X6 = 5                         # acx_resnet_desc.prec only: the ResNet encoder on the plane kernel (precision "bf16x6")
PREC_F32X6_LN16 = 6                     # acx_vit_encode_ln16 only: PREC_F32X6 with the LayerNorm-fed products on fp16 planes (what "auto" resolves to)
PREC_F32X6_R16 = 7                      # acx_vit_encode_r16 only: PREC_F32X6_LN16 with out-proj and c_proj on fp16 planes too ("auto", every proof passing)
PREC_F32X6_QKV16 = 8                    # acx_vit_encode_qkv16 only: PREC_F32X6_R16 with q | k | v as fp16 planes into the three-product planes attention
PREC_F16X3S = 9                         # PREC_F16X3 on every ViT sequence length: the streaming fp16 planes attention outside 193..208 tokens (precision "f16x3s")
ACT_NONE, ACT_QUICKGELU, ACT_LEAKYRELU, ACT_RELU, ACT_RESRELU = 0, 1, 2, 3, 4
ACT_GELU = 5                            # the exact GELU 0.5 x (1 + erf(x / sqrt 2)): CLIP checkpoints not trained with QuickGELU
AMAP_IDENTITY, AMAP_CONV3X3, AMAP_TESTTILE, AMAP_TILETABLE = 0, 1, 2, 3
NORM_LAYER, NORM_CHAN = 0, 1
OPT_RING_MIN_TILES, OPT_SK_MAX_M, OPT_TN_P256_MIN_ROWS, OPT_X6_CUS, OPT_X6_TAIL_SPLIT = 1, 2, 3, 4, 5
OPT_X6_STRIP_TAIL, OPT_X6_MIN_TILES, OPT_LN_RIDER, OPT_ATTN_F32IN, OPT_CLS_FOLD = 6, 7, 8, 9, 10
ACX_F64, ACX_I64 = 16, 17                              # element types of the collectives only (acx_allreduce / acx_allgather)
COMM_SUM, COMM_MAX, COMM_MIN = 0, 1, 2
COMM_ID_BYTES = 128
# acx_seq_attention_bwd_route / acx_axial_attention_route: the kernel route a shape takes (include/acx.h ACX_SAB_ROUTE_* / ACX_AXF_ROUTE_*)
SAB_ROUTE_UNSUPPORTED, SAB_ROUTE_TEXT_MFMA, SAB_ROUTE_TEXT_BLOCK, SAB_ROUTE_TEXT_ROWS = 0, 1, 2, 3
SAB_ROUTE_AXIAL_MFMA, SAB_ROUTE_AXIAL_MFMA_PADDED, SAB_ROUTE_GENERIC = 4, 5, 6
AXF_ROUTE_UNSUPPORTED, AXF_ROUTE_PADDED_MFMA, AXF_ROUTE_EXACT_MFMA, AXF_ROUTE_THREAD_PER_ROW = 0, 1, 2, 3
# acx_attention_route (include/acx.h ACX_ATTN_ROUTE_*); a negative answer is acx_attention's error code for the shape
ATTN_ROUTE_BLOCK32, ATTN_ROUTE_STREAM16, ATTN_ROUTE_STREAM16_QB = 1, 2, 3
# acx_attention_hd_route (include/acx.h ACX_ATTN_HD_ROUTE_*): head dimension 80
ATTN_HD_ROUTE_STREAM, ATTN_HD_ROUTE_STREAM_QB = 1, 2
# acx_gemm_route: the route function of csrc/acx_gemm.hip that takes a descriptor (include/acx.h ACX_GEMM_ROUTE_*)
GEMM_ROUTE_NONE, GEMM_ROUTE_X6_TAIL_SPLIT, GEMM_ROUTE_SK, GEMM_ROUTE_X6, GEMM_ROUTE_S64, GEMM_ROUTE_P256, GEMM_ROUTE_W8 = 0, 1, 2, 3, 4, 5, 6
GEMM_ROUTE_W8_CONV, GEMM_ROUTE_RING, GEMM_ROUTE_P8, GEMM_ROUTE_DMA_CONV, GEMM_ROUTE_DMA, GEMM_ROUTE_GENERIC = 7, 8, 9, 10, 11, 12
GEMM_REDUCE_NONE, GEMM_REDUCE_LAUNCH, GEMM_REDUCE_COUNTERS = 0, 1, 2
# acx_gemm_tn_route / acx_gemm_tn_x6_route (include/acx.h ACX_TN_ROUTE_*); reduce: 0 none, 1 the reduce launch, 2 images for the caller
TN_ROUTE_NONE, TN_ROUTE_W8, TN_ROUTE_P256, TN_ROUTE_X6_256x256, TN_ROUTE_X6_256x128, TN_ROUTE_X6_128x256 = 0, 1, 2, 3, 4, 5
# acx_transformer_plan: a layer's record (include/acx.h ACX_TF_LN_* / ACX_TF_GEMM_* / ACX_TF_BUF_* / ACX_TF_ATT_*)
TF_LN_ROWS, TF_LN_PLANES, TF_LN_RIDDEN, TF_LN_CLS = 0, 1, 2, 3
TF_GEMM_ROWS, TF_GEMM_X6 = 0, 1
TF_BUF_NONE, TF_BUF_SPLITK, TF_BUF_H, TF_BUF_QKV, TF_BUF_MLP = 0, 1, 2, 3, 4
TF_ATT_F32, TF_ATT_BF16, TF_ATT_X3_PANEL, TF_ATT_P3N, TF_ATT_P3F, TF_ATT_CLS, TF_ATT_CLS_FOLD, TF_ATT_S16 = 0, 1, 2, 3, 4, 5, 6, 7
TF_ATT_HD_F32, TF_ATT_HD_X3_PANEL, TF_ATT_HD_CLS = 8, 9, 10          # width == 80 heads


class GemmDesc(C.Structure):
    _fields_ = [
        ("A", c_void_p), ("W", c_void_p), ("C", c_void_p),
        ("M", c_int32), ("N", c_int32), ("K", c_int32),
        ("lda", c_int32), ("ldw", c_int32), ("ldc", c_int32),
        ("a_dtype", c_int32), ("c_dtype", c_int32), ("prec", c_int32),
        ("bias", c_void_p), ("act", c_int32),
        ("residual", c_void_p), ("ldr", c_int32),
        ("a_sub", c_void_p),
        ("amap", c_int32), ("gn", c_int32), ("gl", c_int32), ("cin", c_int32), ("seg", c_int32),
        ("pos0", c_void_p), ("pos1", c_void_p),
        ("workspace", c_void_p), ("workspace_bytes", c_size_t),
        ("zero_page", c_void_p), ("a_act", c_int32), ("gelu_grad_of", c_void_p), ("ldg", c_int32),
        ("a_norm_w", c_void_p), ("a_norm_b", c_void_p), ("a_norm_eps", c_float),
        ("counters", c_void_p), ("n_counters", c_int32),
        ("tile_table", c_void_p),
        ("pairs", c_int32), ("panels", c_int32), ("a_plane_stride", c_int64), ("w_plane_stride", c_int64),
        ("c_plane_rows", c_int64), ("out_scale", c_float), ("c_scale", c_float),
    ]


class GemmScratch(C.Structure):   # acx_gemm_scratch_t: what acx_gemm_scratch tells the caller to bring
    _fields_ = [("workspace_bytes", c_size_t), ("counters", c_int32)]


class GemmRoute(C.Structure):     # acx_gemm_route_t: the route acx_gemm takes, its K pieces, how they are summed, the launch's tiles
    _fields_ = [("route", c_int32), ("ksplit", c_int32), ("reduce", c_int32), ("reserved", c_int32), ("tiles", c_int64)]


class GemmTnRoute(C.Structure):   # acx_gemm_tn_route_t: the kernel acx_gemm_tn* / acx_gemm_tn_x6 runs, its row ranges, who sums them
    _fields_ = [(n, c_int32) for n in ("kernel", "splits", "rows_per_split", "tiles", "reduce", "clears_zero_page")]


class TfProduct(C.Structure):     # acx_tf_product_t: one of a layer's four products as the transformer driver runs it
    _fields_ = [(n, c_int32) for n in ("kernel", "c_dtype", "scratch", "ln_job")]


class TfLayerPlan(C.Structure):   # acx_tf_layer_plan_t: what the transformer driver launches for one layer
    # (`reserved`: the record's last word under the name it had while it was always 0 -- acx_tf_layer_plan_t.att_out_dtype, F16X2P where
    # the attention writes fp16 planes, PREC_F32X6_R16 only)
    _fields_ = [(n, c_int32) for n in ("ln1", "ln1_dtype", "ln2", "ln2_dtype")] + \
               [(n, TfProduct) for n in ("in_proj", "out_proj", "fc", "proj")] + \
               [(n, c_int32) for n in ("att", "att_products", "split_att", "split_mlp", "pruned", "reserved")]


class LnJob(C.Structure):    # acx_ln_job: the LayerNorm acx_gemm_ln runs on the product's output rows
    _fields_ = [("w", c_void_p), ("b", c_void_p), ("y", c_void_p), ("y_dtype", c_int32), ("eps", c_float), ("mode", c_int32),
                ("y_scale", c_float)]


class BlockWeights(C.Structure):
    _fields_ = [(n, c_void_p) for n in (
        "ln1_w", "ln1_b", "ln2_w", "ln2_b", "in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b",
        "fc_w", "fc_b", "proj_w", "proj_b",
        "in_proj_w_bf16", "out_proj_w_bf16", "fc_w_bf16", "proj_w_bf16")]


class VitWeights(C.Structure):
    _fields_ = [
        ("conv1_w", c_void_p), ("conv1_w_bf16", c_void_p),
        ("class_embedding", c_void_p), ("positional_embedding", c_void_p),
        ("ln_pre_w", c_void_p), ("ln_pre_b", c_void_p), ("ln_post_w", c_void_p), ("ln_post_b", c_void_p),
        ("proj_t", c_void_p), ("proj_t_bf16", c_void_p),
        ("blocks", C.POINTER(BlockWeights)),
    ]


class CurveResult(C.Structure):          # == struct acx_curve_result (56 bytes, device memory)
    _fields_ = [("auroc", C.c_double), ("ap", C.c_double), ("n_pos", c_int64), ("n_neg", c_int64),
                ("n_distinct", c_int64), ("opt_index", c_int64), ("opt_threshold", c_float), ("pad", c_float)]


class TnProblem(C.Structure):          # == struct acx_tn_problem
    _fields_ = [("A", c_void_p), ("B", c_void_p), ("C", c_void_p), ("b_sub", c_void_p), ("M", c_int32), ("N1", c_int32),
                ("N2", c_int32), ("lda", c_int32), ("ldb", c_int32), ("reserved", c_int32)]


class PrepSeg(C.Structure):            # == struct acx_prep_seg
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("rows", c_int32), ("cols", c_int32), ("src_ld", c_int32),
                ("dst_ld", c_int32), ("transpose", c_int32), ("reserved", c_int32)]


class VitDesc(C.Structure):            # == struct acx_vit_desc (act: 0 / ACT_QUICKGELU or ACT_GELU; ctypes zeroes what is not given)
    _fields_ = [(n, c_int32) for n in ("resolution", "patch", "width", "layers", "heads", "embed_dim", "prec", "act")]


class ResnetConv(C.Structure):          # == struct acx_resnet_conv
    _fields_ = [("w", c_void_p), ("b", c_void_p), ("w3", c_void_p)]


class ResnetBlock(C.Structure):         # == struct acx_resnet_block
    _fields_ = [("conv1", ResnetConv), ("conv2", ResnetConv), ("conv3", ResnetConv), ("downsample", ResnetConv)]


class ResnetWeights(C.Structure):       # == struct acx_resnet_weights
    _fields_ = [("stem", ResnetConv * 3), ("blocks", C.POINTER(ResnetBlock)), ("positional_embedding", c_void_p),
                ("q_w", c_void_p), ("q_b", c_void_p), ("kv_w", c_void_p), ("kv_b", c_void_p), ("c_w", c_void_p), ("c_b", c_void_p),
                ("kv_w3", c_void_p)]


class ResnetBn(C.Structure):            # == struct acx_resnet_bn
    _fields_ = [("weight", c_void_p), ("bias", c_void_p), ("running_mean", c_void_p), ("running_var", c_void_p),
                ("num_batches_tracked", c_void_p)]


class ResnetBlockBn(C.Structure):       # == struct acx_resnet_block_bn
    _fields_ = [("bn1", ResnetBn), ("bn2", ResnetBn), ("bn3", ResnetBn), ("downsample", ResnetBn)]


class ResnetTrainBn(C.Structure):       # == struct acx_resnet_train_bn
    _fields_ = [("stem", ResnetBn * 3), ("blocks", C.POINTER(ResnetBlockBn)), ("eps", c_float), ("momentum", c_float)]


class ResnetDesc(C.Structure):          # == struct acx_resnet_desc
    _fields_ = [("resolution", c_int32), ("width", c_int32), ("layers", c_int32 * 4), ("heads", c_int32), ("output_dim", c_int32),
                ("prec", c_int32)]


class JpegInfo(C.Structure):            # == struct acx_jpeg_info
    _fields_ = [(n, c_int32) for n in ("width", "height", "ncomp", "hmax", "vmax", "mcus_x", "mcus_y", "restart_interval")] + \
               [(n, c_int32 * 4) for n in ("comp_h", "comp_v", "comp_tq", "comp_td", "comp_ta", "comp_width", "comp_height",
                                           "blocks_wide", "blocks_high")] + \
               [("coef_offset", c_int64 * 4), ("coef_elems", c_int64), ("scan_offset", c_int64),
                ("qtab", (C.c_uint16 * 64) * 4), ("qtab_present", C.c_uint8 * 4), ("huff_present", (C.c_uint8 * 4) * 2),
                ("huff_bits", ((C.c_uint8 * 17) * 4) * 2), ("huff_vals", ((C.c_uint8 * 256) * 4) * 2)]


class VizGeom(C.Structure):             # == struct acx_viz_geom
    _fields_ = [(n, c_int32) for n in ("Hc", "Wc", "H", "W", "fx", "fy", "fw", "fh", "border", "bx", "by", "bh", "bar_pitch", "bar_w",
                                       "C1", "sx", "sy", "sw", "sh", "cursor_w", "T")] + [("threshold", c_float)]


class JpegHuff(C.Structure):            # == struct acx_jpeg_huff
    _fields_ = [("present", (C.c_uint8 * 4) * 2), ("bits", ((C.c_uint8 * 17) * 4) * 2), ("vals", ((C.c_uint8 * 256) * 4) * 2),
                ("td", C.c_uint8 * 4), ("ta", C.c_uint8 * 4)]


_SIGS = {
    "acx_version": (C.c_int, []),
    "acx_create": (C.c_int, [C.POINTER(c_void_p), C.c_int]),
    "acx_destroy": (None, [c_void_p]),
    "acx_last_error": (C.c_char_p, [c_void_p]),
    "acx_set_option": (C.c_int, [c_void_p, c_int32, c_int64]),
    "acx_get_option": (C.c_int, [c_void_p, c_int32, C.POINTER(c_int64)]),
    "acx_gemm": (C.c_int, [c_void_p, C.POINTER(GemmDesc), c_void_p]),
    "acx_gemm_scratch": (C.c_int, [c_void_p, C.POINTER(GemmDesc), c_int32, C.POINTER(GemmScratch)]),
    "acx_gemm_route": (C.c_int, [c_void_p, C.POINTER(GemmDesc), C.POINTER(GemmRoute)]),
    "acx_gemm_ln": (C.c_int, [c_void_p, C.POINTER(GemmDesc), C.POINTER(LnJob), c_void_p]),
    "acx_gemm_ln_plan": (c_int64, [c_int32, c_int32, c_int32, c_int32, c_int32, C.c_double, C.POINTER(c_int64)]),
    "acx_layernorm": (C.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int32,
                                c_int64, c_int32, c_float, c_int32, c_void_p]),
    "acx_layernorm_scaled": (C.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_float, c_int32,
                                       c_float, c_void_p]),
    "acx_attention": (C.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_int32,
                                c_int32, c_void_p]),
    "acx_attention_route": (C.c_int, [c_void_p, c_int32, c_int32, c_int32]),
    "acx_attention_hd": (C.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "acx_attention_x3_hd": (C.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "acx_attention_cls_hd": (C.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "acx_attention_hd_route": (C.c_int, [c_void_p, c_int32, c_int32, c_int32]),
    "acx_attention_bf16": (C.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p]),
    "acx_attention_x3": (C.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p]),
    "acx_attention_p3": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "acx_attention_p3n": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "acx_attention_p3f": (C.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "acx_attention_p3f16": (C.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_float, c_int32, c_int32, c_int32, c_void_p]),
    "acx_attention_p3h16": (C.c_int, [c_void_p, c_void_p, c_float, c_void_p, c_float, c_int32, c_int32, c_int32, c_void_p]),
    "acx_attention_s16": (C.c_int, [c_void_p, c_void_p, c_float, c_void_p, c_float, c_int32, c_int32, c_int32, c_void_p]),
    "acx_attention_x3_panel": (C.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p]),
    "acx_attention_cls": (C.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p]),
    "acx_attention_cls_fold_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "acx_attention_cls_fold": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                         c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_size_t, c_void_p]),
    "acx_vit_patches": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "acx_vit_embed": (C.c_int, [c_void_p] * 7 + [c_int32, c_int32, c_int32, c_void_p]),
    "acx_resnet_stem_im2col": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    "acx_avgpool2_nhwc": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "acx_attnpool_tokens": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "acx_resnet_workspace_bytes": (c_size_t, [C.POINTER(ResnetDesc), c_int32]),
    "acx_bn_apply_nhwc": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32,
                                    c_int32, c_float, c_int32, c_void_p, c_void_p]),
    "acx_resnet_train_workspace_bytes": (c_size_t, [C.POINTER(ResnetDesc), c_int32]),
    "acx_resnet_encode_train": (C.c_int, [c_void_p, C.POINTER(ResnetDesc), C.POINTER(ResnetWeights), C.POINTER(ResnetTrainBn), c_void_p,
                                          c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "acx_resnet_encode": (C.c_int, [c_void_p, C.POINTER(ResnetDesc), C.POINTER(ResnetWeights), c_void_p, c_int32, c_void_p,
                                    c_void_p, c_size_t, c_void_p]),
    "acx_vit_workspace_bytes": (c_size_t, [C.POINTER(VitDesc), c_int32]),
    "acx_vit_encode": (C.c_int, [c_void_p, C.POINTER(VitDesc), C.POINTER(VitWeights), c_void_p, c_int32, c_void_p,
                                 c_void_p, c_size_t, c_void_p]),
    "acx_vit_encode_ln16": (C.c_int, [c_void_p, C.POINTER(VitDesc), C.POINTER(VitWeights), c_void_p, c_void_p, c_int32, c_void_p,
                                      c_void_p, c_size_t, c_void_p]),
    "acx_vit_encode_r16": (C.c_int, [c_void_p, C.POINTER(VitDesc), C.POINTER(VitWeights), c_void_p, c_void_p, c_int32, c_void_p,
                                     c_void_p, c_size_t, c_void_p]),
    "acx_vit_encode_qkv16": (C.c_int, [c_void_p, C.POINTER(VitDesc), C.POINTER(VitWeights), c_void_p, c_void_p, c_int32, c_void_p,
                                       c_void_p, c_size_t, c_void_p]),
    "acx_transformer_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "acx_transformer_workspace_bytes_prec": (c_size_t, [c_int32, c_int32, c_int32]),
    "acx_transformer_forward": (C.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                          c_int32, C.POINTER(BlockWeights), c_void_p, c_size_t, c_void_p]),
    "acx_transformer_forward_act": (C.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                              c_int32, c_int32, C.POINTER(BlockWeights), c_void_p, c_size_t, c_void_p]),
    "acx_transformer_plan": (C.c_int, [c_void_p] + [c_int32] * 10 + [C.POINTER(TfLayerPlan)]),
    "acx_text_directions": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "acx_selector_project": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32,
                                       c_void_p]),
    "acx_probe_mfma": (C.c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, C.POINTER(C.c_double), c_void_p]),
    "acx_probe_copy": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "acx_split_bf16x3_multi": (C.c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "acx_probe_read": (C.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "acx_comm_unique_id": (C.c_int, [c_void_p, c_size_t]),
    "acx_comm_init": (C.c_int, [c_void_p, c_int32, c_int32, c_void_p]),
    "acx_comm_destroy": (C.c_int, [c_void_p]),
    "acx_comm_info": (C.c_int, [c_void_p, C.POINTER(c_int32), C.POINTER(c_int32)]),
    "acx_allreduce": (C.c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p]),
    "acx_allgather": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    "acx_bn_workspace_bytes": (c_size_t, [c_int64, c_int32]),
    "acx_bn_combine": (C.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "acx_bn_stats": (C.c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "acx_selector_project_stats": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "acx_selector_bn": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32,
                                  c_float, c_void_p]),
    "acx_axial_attention": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                      c_int32, c_void_p]),
    "acx_axial_attention_route": (C.c_int, [c_void_p] + [c_int32] * 6),
    "acx_cls_head": (C.c_int, [c_void_p] * 8 + [c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "acx_cls_head_tiles": (C.c_int, [c_void_p] * 8 + [c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "acx_class_probs": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    "acx_prompt_embed": (C.c_int, [c_void_p] * 6 + [c_int32] * 6 + [c_void_p]),
    "acx_gather_rows": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    "acx_add_bcast": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "acx_concat_features": (C.c_int, [c_void_p] * 5 + [c_int64, c_int32, c_int32, c_int32, c_void_p]),
    "acx_prof_enable": (C.c_int, [c_void_p, C.c_int]),
    "acx_prof_gemm_flops": (C.c_int, [c_void_p, C.POINTER(C.c_double)]),
    "acx_prof_collect": (C.c_int, [c_void_p, C.POINTER(c_int32), C.POINTER(C.c_double)]),
    "acx_prof_gemm_tn": (C.c_int, [c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(c_int32)]),
    "acx_gemm_tn_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "acx_gemm_tn": (C.c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32,
                              c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_size_t, c_void_p]),
    "acx_reduce_rows": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    "acx_layernorm_bwd": (C.c_int, [c_void_p] * 6 + [c_int64, c_int32, c_float, c_int32, c_float, c_void_p, c_void_p]),
    "acx_cls_head_bwd": (C.c_int, [c_void_p] * 10 + [c_int64, c_int32, c_void_p]),
    "acx_act": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    "acx_leaky_grad_planes": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "acx_add": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "acx_transpose": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    "acx_conv_weight_dx": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    "acx_seq_attention_bwd": (C.c_int, [c_void_p] * 4 + [c_int32] * 7 + [c_void_p, c_void_p]),
    "acx_seq_attention_bwd_route": (C.c_int, [c_void_p] + [c_int32] * 8),
    "acx_pos_grad": (C.c_int, [c_void_p] * 5 + [c_int32] * 4 + [c_void_p]),
    "acx_bn_bwd_stats": (C.c_int, [c_void_p] * 4 + [c_int64, c_int32, c_void_p, c_size_t, c_void_p]),
    "acx_bn_bwd_apply": (C.c_int, [c_void_p] * 6 + [c_int32, c_int64, c_int64, c_int32, c_float, c_void_p, c_void_p]),
    "acx_axpby": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_float, c_float, c_void_p]),
    "acx_colsum_partials": (C.c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int32, c_int32, c_void_p]),
    "acx_text_directions_bwd": (C.c_int, [c_void_p] * 5 + [c_int32] * 3 + [c_void_p]),
    "acx_select_idx": (C.c_int, [c_void_p] * 7 + [c_int32] * 7 + [c_void_p]),
    "acx_gather_segments": (C.c_int, [c_void_p] * 4 + [c_int32] * 5 + [c_void_p]),
    "acx_scatter_segments": (C.c_int, [c_void_p] * 4 + [c_int32] * 5 + [c_void_p]),
    "acx_mil_loss_one": (C.c_int, [c_void_p] * 13 + [c_size_t] + [c_int32] * 6 + [c_void_p, c_void_p, c_void_p, c_void_p]),
    "acx_mil_loss_bn": (C.c_int, [c_void_p] * 14 + [c_size_t, c_void_p, c_size_t] + [c_int32] * 6 + [c_void_p, c_void_p, c_void_p, c_void_p]),
    "acx_mil_loss_bn_fits": (C.c_int, [c_void_p] + [c_int32] * 5),
    "acx_selector_tail": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int32] + [c_void_p] * 7 + [c_float, c_float, c_void_p, c_int64] +
                          [c_void_p] * 6 + [c_int32] * 7 + [c_float, c_void_p]),
    "acx_selector_tail_fits": (C.c_int, [c_void_p] + [c_int32] * 6),
    "acx_text_directions_bwd_parts": (C.c_int, [c_void_p] * 4 + [c_int32, c_int64, c_void_p] + [c_int32] * 3 + [c_void_p]),
    "acx_adamw": (C.c_int, [c_void_p] * 5 + [c_int64] + [c_float] * 5 + [c_int32, c_void_p]),
    "acx_multi_axpy": (C.c_int, [c_void_p, c_int32, C.POINTER(c_void_p), C.POINTER(c_void_p), C.POINTER(c_int64), c_float, c_void_p]),
    "acx_adamw_multi": (C.c_int, [c_void_p, c_int32] + [C.POINTER(c_void_p)] * 4 + [C.POINTER(c_int64), C.POINTER(C.c_double),
                                  C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double, c_int32, c_void_p]),
    "acx_row_parts": (c_int64, [c_int64]),
    "acx_prep_multi": (C.c_int, [c_void_p, c_int32, c_void_p, c_void_p]),
    "acx_multi_copy": (C.c_int, [c_void_p, c_int32, C.POINTER(c_void_p), C.POINTER(c_void_p), C.POINTER(c_int64), c_void_p]),
    "acx_adamw_hyper": (C.c_int, [c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_double, c_int32,
                                  C.POINTER(c_float)]),
    "acx_adamw_multi_dev": (C.c_int, [c_void_p, c_int32] + [C.POINTER(c_void_p)] * 4 + [C.POINTER(c_int64), c_void_p, c_float,
                                      C.c_double, C.c_double, C.c_double, c_void_p]),
    "acx_grad_norm_workspace_bytes": (c_size_t, [c_int32, c_int64]),
    "acx_grad_norm": (C.c_int, [c_void_p, c_int32, C.POINTER(c_void_p), C.POINTER(c_int64), c_float, c_float, c_void_p, c_void_p,
                                c_size_t, c_void_p]),
    "acx_adamw_multi_dev_clip": (C.c_int, [c_void_p, c_int32] + [C.POINTER(c_void_p)] * 4 + [C.POINTER(c_int64), c_void_p, c_float,
                                           C.c_double, C.c_double, C.c_double, c_void_p, c_float, c_void_p]),
    "acx_clip_grads": (C.c_int, [c_void_p, c_int32, C.POINTER(c_void_p), C.POINTER(c_int64), c_float, c_void_p, c_float, c_void_p]),
    "acx_bn_pack": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "acx_bn_running_update": (C.c_int, [c_void_p] * 6 + [c_int32, c_float, c_float, c_void_p]),
    "acx_fill_f32": (C.c_int, [c_void_p, c_void_p, c_int64, c_float, c_void_p]),
    "acx_gemm_tn_group_workspace_bytes": (c_size_t, [c_int32, c_void_p]),
    "acx_gemm_tn_group": (C.c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "acx_colsum_fused_part_bytes": (c_size_t, [c_int64, c_int32]),
    "acx_colsum_fused": (C.c_int, [c_void_p, c_void_p, c_int32, c_int64, c_int32, c_void_p, c_void_p, c_size_t, c_void_p, c_float, c_void_p]),
    "acx_colsum_fused_group": (C.c_int, [c_void_p, c_int32, C.POINTER(c_void_p), C.POINTER(c_int32), C.POINTER(c_int64),
                                         C.POINTER(c_int32), C.POINTER(c_void_p), C.POINTER(c_void_p), c_void_p, c_int32, c_void_p]),
    "acx_reduce_rows_group": (C.c_int, [c_void_p, c_int32, C.POINTER(c_void_p), C.POINTER(c_void_p), C.POINTER(c_int32),
                                        C.POINTER(c_int32), c_void_p]),
    "acx_gemm_tn_zp": (C.c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                 c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_size_t, c_void_p, c_void_p]),
    "acx_split_f16x2": (C.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_float, c_int32, c_void_p]),
    "acx_gemm_tn_parts": (C.c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                    c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_size_t, c_void_p, C.POINTER(c_int32), c_void_p]),
    "acx_gemm_tn_x6_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "acx_gemm_tn_x6": (C.c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_int64, c_int32, c_void_p, c_int32, c_int32, c_int32,
                                 c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_size_t, c_void_p, c_void_p]),
    "acx_gemm_tn_route": (C.c_int, [c_void_p] + [c_int32] * 12 + [c_size_t, c_int32, c_int32, C.POINTER(GemmTnRoute)]),
    "acx_gemm_tn_x6_route": (C.c_int, [c_void_p] + [c_int32] * 11 + [c_size_t, c_int32, C.POINTER(GemmTnRoute)]),
    "acx_ctx_grad": (C.c_int, [c_void_p] * 3 + [c_int32] * 5 + [c_void_p]),
    "acx_scatter_rows": (C.c_int, [c_void_p] * 4 + [c_int64, c_int32, c_void_p]),
    "acx_preprocess_frames": (C.c_int, [c_void_p] * 6 + [c_int32, c_void_p, c_void_p, c_int32] + [c_int32] * 5 +
                              [C.POINTER(c_float), C.POINTER(c_float), c_void_p]),
    "acx_preprocess_crops": (C.c_int, [c_void_p] * 6 + [c_int32, c_void_p, c_void_p, c_int32] + [c_int32] * 7 +
                             [C.POINTER(c_int32), C.POINTER(c_float), C.POINTER(c_float), c_void_p]),
    "acx_cast_bf16": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "acx_split_bf16x3": (C.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p]),
    "acx_split_bf16x3_panel": (C.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p]),
    "acx_colsum": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    "acx_sort_workspace_bytes": (c_int64, [c_int64]),
    "acx_sort_pairs_batched": (C.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32, c_int32,
                                         c_void_p, c_int64, c_void_p]),
    "acx_sort_pairs": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_int64,
                                 c_void_p]),
    "acx_clf_curve_workspace_bytes": (c_int64, [c_int64]),
    "acx_clf_curve_batched": (C.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, C.POINTER(c_int32),
                                        C.POINTER(c_int32), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "acx_clf_curve": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_int64, c_void_p]),
    "acx_curve_decimate_workspace_bytes": (c_int64, [c_int64]),
    "acx_curve_decimate": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int64,
                                     c_void_p]),
    "acx_test_counts": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p,
                                  c_void_p, c_void_p]),
    "acx_score_events_workspace_bytes": (c_int64, [c_int64, c_int64, c_int32]),
    "acx_score_events": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_float, c_float,
                                   c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "acx_sample_segments": (C.c_int, [c_void_p] * 7 + [c_int32] * 6 + [c_void_p]),
    "acx_tile_videos": (C.c_int, [c_void_p] * 9 + [c_int32, c_int64] + [c_int32] * 5 + [c_void_p]),
    "acx_sample_segments_f16": (C.c_int, [c_void_p] * 7 + [c_int32] * 6 + [c_void_p]),
    "acx_tile_videos_f16": (C.c_int, [c_void_p] * 9 + [c_int32, c_int64] + [c_int32] * 5 + [c_void_p]),
    "acx_cast_rows_f16": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int64, c_void_p, c_void_p]),
    "acx_expand_rows_f16": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    "acx_jpeg_parse": (C.c_int, [c_void_p, c_size_t, c_void_p]),
    "acx_jpeg_entropy_decode": (C.c_int, [c_void_p, c_size_t, c_void_p, c_void_p, c_size_t]),
    "acx_jpeg_scan_pack": (C.c_int, [c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "acx_jpeg_entropy_decode_dev": (C.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p] + [c_int32] * 6 +
                                    [c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    "acx_jpeg_reconstruct": (C.c_int, [c_void_p, c_void_p, c_void_p] + [c_int32] * 6 + [c_void_p, c_void_p, c_void_p]),
    "acx_viz_compose": (C.c_int, [c_void_p] * 8 + [c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "acx_jpeg_forward": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "acx_jpeg_entropy_encode": (c_int64, [c_void_p, c_size_t, c_void_p, c_int32, c_int32, c_void_p, c_size_t]),
    "acx_jpeg_encode_bound": (c_int64, [c_int32, c_int32]),
    "acx_jpeg_encode_header": (c_int64, [c_void_p, c_int32, c_int32, c_void_p, c_size_t]),
    "acx_jpeg_entropy_encode_dev_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "acx_jpeg_entropy_encode_dev": (C.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64,
                                              c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}

# entry points added by later translation units register themselves here (name -> signature)
EXTRA_SIGS: dict = {}

_lock = threading.Lock()
_lib = None
_ctxs: dict = {}


class AcxError(RuntimeError):
    pass


def declared_symbols():
    return sorted(set(_SIGS) | set(EXTRA_SIGS))


def lib() -> C.CDLL:
    """Loads (building if the in-tree binary is missing or stale and hipcc is present) libacx.so."""
    global _lib
    with _lock:
        if _lib is None:
            path = os.environ.get("ACX_LIB_PATH") or _build.LIB
            if os.environ.get("ACX_LIB_PATH"):
                pass
            elif not os.path.exists(path) or (os.environ.get("ACX_AUTOBUILD") == "1" and _build._stale()):
                # The prebuilt in-tree binary is used as it is (several ranks may import concurrently and file
                # times do not survive a snapshot copy); rebuilding is explicit: __graft_entry__.build(),
                # `python -m anomalyclip_amd._build`, or ACX_AUTOBUILD=1 for development.
                if not os.path.exists(_build.HIPCC):
                    raise AcxError(f"libacx.so not found at {path} and hipcc is not available to build it; "
                                   f"there is no fallback compute path")
                path = _build.build(verbose=False)
            # torch first: its bundled HIP runtime must be the one libacx.so's libamdhip64 dependency resolves to.  Loaded
            # the other way round (libacx.so, then torch) the process ends up with two HIP runtimes and the one libacx sees
            # reports "0 devices" while torch.cuda.is_available() is true (__graft_entry__.build() followed by smoke()).
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
            try:
                L = C.CDLL(path)
            except OSError as e:
                raise AcxError(f"libacx.so could not be loaded from {path}: {e}. There is no fallback path: "
                               f"build it with `python -m anomalyclip_amd._build`.") from e
            for name, (res, args) in {**_SIGS, **EXTRA_SIGS}.items():
                try:
                    fn = getattr(L, name)
                except AttributeError as e:
                    if os.environ.get("ACX_LIB_PATH"):
                        # an A/B library built from another commit (tools/ab_x6.sh) may lack an entry point this tree declares:
                        # calling it is the error, loading the library is not
                        def _missing(*_a, _name=name, _path=path):
                            raise AcxError(f"{_path} (ACX_LIB_PATH) does not export {_name}")
                        setattr(L, name, _missing)
                        continue
                    raise AcxError(f"libacx.so does not export {name}") from e
                fn.restype = res
                fn.argtypes = args
            _lib = L
        return _lib


def exports(name: str) -> bool:
    """whether the loaded library has entry point `name` (an ACX_LIB_PATH library of another commit may not)"""
    return isinstance(getattr(lib(), name, None), C._CFuncPtr)


def ctx(device: int = 0) -> int:
    """One acx context per device."""
    L = lib()
    with _lock:
        if device not in _ctxs:
            h = c_void_p()
            rc = L.acx_create(C.byref(h), device)
            if rc != 0:
                raise AcxError(f"acx_create({device}) failed [{rc}]: {L.acx_last_error(None).decode()}")
            _ctxs[device] = h.value
        return _ctxs[device]


def check(rc: int, handle) -> None:
    if rc != 0:
        raise AcxError(f"libacx error {rc}: {lib().acx_last_error(handle).decode()}")
