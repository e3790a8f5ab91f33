"""No device: the ResNet encoders' precision "bf16x6" (ACX_PREC_BF16X6) where it needs no GPU -- the precision names and their
refusals, acx_resnet_workspace_bytes (the f32 answer unchanged, from the carve formula restated here; the new precision larger),
acx_resnet_encode's argument errors before any launch, acx_gemm_scratch on the general convolution map and extract's parser."""
import ctypes as C

import pytest

from anomalyclip_amd import _lib as L
from anomalyclip_amd import extract as X
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd.components.anomaly_clip import AnomalyCLIP
from anomalyclip_amd.components.clip_resnet import RESNET_PRECISIONS, check_resnet_precision

GEOMS = {"RN50": IW.RN50, "RN101": IW.RN101, "RN50x4": IW.RN50X4, "RN50x16": IW.RN50X16, "RN50x64": IW.RN50X64}


def _desc(geom, prec):
    return L.ResnetDesc(geom.image_resolution, geom.vision_width, (C.c_int32 * 4)(*geom.vision_layers), geom.resnet_heads,
                        geom.embed_dim, prec)


def _cp(c):
    return (c + 31) // 32 * 32


def _al(x):
    return (x + 255) // 256 * 256


def f32_workspace_ref(geom, frames):
    """acx_resnet_workspace_bytes for the f32 kernels, restated: the largest activation per frame, the internal batch that keeps
    it below 2^31 bytes (at most 512 frames), nine 256-byte aligned f32 buffers"""
    R, w = geom.image_resolution, geom.vision_width
    G1, E, HW = R // 2, w * 32, (R // 32) ** 2
    m = max(G1 * G1 * _cp(w), G1 * G1 * 32)
    H, inpl = G1 // 2, w
    for li, blocks in enumerate(geom.vision_layers):
        planes = w << li
        for j in range(blocks):
            m = max(m, H * H * _cp(max(planes, inpl)))
            if li > 0 and j == 0:
                H //= 2
            m = max(m, H * H * 4 * planes)
            inpl = 4 * planes
    fb = min(512, max(1, (1 << 31) // (m * 4)))
    fb = min(fb, frames)
    floats = [fb * G1 * G1 * 32] + [fb * m] * 5 + [fb * (HW + 1) * E, fb * (HW + 1) * 3 * E, fb * E]
    return sum(_al(4 * n) for n in floats), fb, m, (HW + 1) * E


def test_precision_names():
    assert RESNET_PRECISIONS["bf16x6"] == L.PREC_BF16X6 == 5
    assert L.PREC_BF16X6 not in (L.PREC_F32, L.PREC_F32X6) and RESNET_PRECISIONS["auto"] == RESNET_PRECISIONS["f32x6"] == L.PREC_F32X6
    for arch, geom in GEOMS.items():
        check_resnet_precision("bf16x6", arch, geom.vision_width)
    for bad in ("bf16", "bf16x3", "f16x3"):
        with pytest.raises(ValueError, match="bf16x6"):                 # the refusal names what the ResNets do run
            check_resnet_precision(bad, "RN50", 64)


def test_vit_arch_refuses_bf16x6_and_names_auto():
    with pytest.raises(ValueError, match="'auto' already is that arithmetic"):
        AnomalyCLIP(arch="ViT-B/16", precision="bf16x6", labels_key="ucf", emb_size=256, depth=1, heads=8, dim_heads=None,
                    num_segments=32, seg_length=16, concat_features=False, normal_id=7, stride=1, select_idx_dropout_topk=0.7,
                    select_idx_dropout_bottomk=0.7, ncrops=1, num_topk=3, num_bottomk=3)


@pytest.mark.parametrize("arch", list(GEOMS))
@pytest.mark.parametrize("frames", [1, 2, 64, 512])
def test_workspace_bytes(arch, frames):
    geom = GEOMS[arch]
    lib = L.lib()
    want, fb, m, tok = f32_workspace_ref(geom, frames)
    for prec in (L.PREC_F32, L.PREC_F32X6):
        d = _desc(geom, prec)
        assert lib.acx_resnet_workspace_bytes(C.byref(d), frames) == want, prec
    d = _desc(geom, L.PREC_BF16X6)
    got = lib.acx_resnet_workspace_bytes(C.byref(d), frames)
    # three buffers of three bf16 planes of the largest activation (or the attention pool's tokens) and one 256-byte zero page
    assert got == want + 3 * _al(3 * fb * max(m, tok) * 2) + 256 and got > want


def test_workspace_bytes_refuses_other_precisions():
    lib = L.lib()
    for prec in (L.PREC_BF16, L.PREC_F32X3, L.PREC_F16X3, 6, -1):
        d = _desc(IW.RN50, prec)
        assert lib.acx_resnet_workspace_bytes(C.byref(d), 2) == 0, prec


def test_encode_argument_errors_before_any_launch():
    """null pointers: ACX_E_BADARG; a precision the driver does not know: ACX_E_UNSUPPORTED -- both decided on the host (the
    'device' pointers here are never dereferenced: there is no device)"""
    lib = L.lib()
    d = _desc(IW.RN50, L.PREC_BF16X6)
    w = L.ResnetWeights()
    arr = (L.ResnetBlock * 16)()
    w.blocks = C.cast(arr, C.POINTER(L.ResnetBlock))
    p = 0x10000
    call = lambda dd, ww, fr, out, ws: lib.acx_resnet_encode(None, dd, ww, fr, 2, out, ws, 1 << 20, None)   # noqa: E731
    assert call(None, C.byref(w), p, p, p) == -1
    assert call(C.byref(d), None, p, p, p) == -1
    assert call(C.byref(d), C.byref(w), None, p, p) == -1
    assert call(C.byref(d), C.byref(w), p, None, p) == -1
    assert call(C.byref(d), C.byref(w), p, p, None) == -1
    w0 = L.ResnetWeights()                                               # no block table
    assert call(C.byref(d), C.byref(w0), p, p, p) == -1
    for prec in (L.PREC_BF16, L.PREC_F32X3, 6):
        bad = _desc(IW.RN50, prec)
        assert call(C.byref(bad), C.byref(w), p, p, p) == -2, prec
    # a workspace that is too small is refused before the zero page is cleared or anything is launched
    assert call(C.byref(d), C.byref(w), p, p, p) == -4
    assert lib.acx_resnet_encode(None, C.byref(d), C.byref(w), p, 0, p, p, 0, None) == 0          # no frames: nothing to do


def _conv_desc(M, N, cin, gn, gl, act=L.ACT_RELU):
    d = L.GemmDesc()
    d.A, d.W, d.C = 0x10000, 0x20000, 0x30000                           # (never dereferenced by the query)
    d.M, d.N, d.K = M, N, 9 * cin
    d.lda, d.ldw, d.ldc = cin, 9 * cin, N
    d.a_dtype, d.c_dtype, d.prec, d.pairs = L.ACX_BF16, L.ACX_F32, L.PREC_BF16, 6
    d.a_plane_stride, d.w_plane_stride = M * cin * 2, N * 9 * cin * 2
    d.amap, d.gn, d.gl, d.cin, d.act = L.AMAP_CONV3X3, gn, gl, cin, act
    d.zero_page = 0x40000
    return d


@pytest.mark.parametrize("M,gn,gl", [(147, 7, 7), (162, 9, 9), (120, 5, 12), (972, 18, 18), (3136, 56, 56)])
def test_gemm_scratch_on_the_general_convolution_map(M, gn, gl):
    """a convolution off the power-of-two grids never splits K (identical frames stay bit-identical wherever they sit): nothing to
    bring, whatever the activation; the power-of-two grid with the ReLU epilogue neither; without it the answer is the parent's"""
    out = L.GemmScratch()
    for act in (L.ACT_RELU, L.ACT_NONE):
        d = _conv_desc(M, 64, 64, gn, gl, act)
        out.workspace_bytes, out.counters = 12345, 7
        assert L.lib().acx_gemm_scratch(None, C.byref(d), 1, C.byref(out)) == 0
        assert (int(out.workspace_bytes), int(out.counters)) == (0, 0)
    d = _conv_desc(256, 64, 64, 16, 16, L.ACT_RELU)
    assert L.lib().acx_gemm_scratch(None, C.byref(d), 1, C.byref(out)) == 0 and out.workspace_bytes == 0
    d = _conv_desc(256, 64, 64, 16, 16, L.ACT_NONE)                      # one tile, K = 576: split 16 ways (x6_split_scratch_bytes)
    assert L.lib().acx_gemm_scratch(None, C.byref(d), 1, C.byref(out)) == 0 and out.workspace_bytes == 16 * 256 * 64 * 4


def test_gemm_scratch_relu_epilogues_bring_nothing():
    for act, res in ((L.ACT_RELU, 0), (L.ACT_RESRELU, 0x50000)):
        d = L.GemmDesc()
        d.A, d.W, d.C = 0x10000, 0x20000, 0x30000
        d.M, d.N, d.K = 49, 2048, 512
        d.lda, d.ldw, d.ldc, d.ldr = 512, 512, 2048, 2048
        d.a_dtype, d.c_dtype, d.prec, d.pairs = L.ACX_BF16, L.ACX_F32, L.PREC_BF16, 6
        d.a_plane_stride, d.w_plane_stride = 49 * 512 * 2, 2048 * 512 * 2
        d.act, d.residual = act, res
        out = L.GemmScratch()
        out.workspace_bytes = 1
        assert L.lib().acx_gemm_scratch(None, C.byref(d), 1, C.byref(out)) == 0 and out.workspace_bytes == 0


def test_extract_parser_accepts_bf16x6(tmp_path):
    a = X._parser().parse_args(["--arch", "RN50", "--weights", "w", "--frames-root", "f", "--out-root", "o", "--precision", "bf16x6"])
    assert a.precision == "bf16x6"
    (tmp_path / "w.pt").write_bytes(b"")
    (tmp_path / "frames").mkdir()
    argv = ["--weights", str(tmp_path / "w.pt"), "--frames-root", str(tmp_path / "frames"), "--out-root", str(tmp_path / "o"),
            "--precision", "bf16x6"]
    assert X.parse_args(["--arch", "RN50x4"] + argv).precision == "bf16x6"
    with pytest.raises(SystemExit) as e:                                 # a ViT: argparse's exit, the message names "auto"
        X.parse_args(["--arch", "ViT-B/16"] + argv)
    assert e.value.code == 2


def test_resnet_plane_kernels_use_no_scratch():
    """gemm_x6_rn_kernel -- the plane kernel's body with the ReLU epilogues and the general convolution map -- in the library as
    built: the eight instantiations the driver and acx_gemm use (C_MODE, ACT, RES, CONV), whole-register-file kernels (one wave
    per SIMD) without scratch or spills"""
    import re
    from anomalyclip_amd import _build
    L.lib()
    rows = {tuple(int(x) for x in re.findall(r"Li(\d+)E", k.split("gemm_x6_rn_kernelI")[1])): v
            for k, v in _build.kernel_resources().items() if "gemm_x6_rn_kernel" in k}
    assert all(t[4:] == (0, 0, 4, 0, 0, 0) for t in rows), sorted(rows)            # NT, six products, whole tiles, no rider
    assert sorted(t[:4] for t in rows) == [(0, 0, 0, 2), (0, 3, 0, 0), (0, 3, 0, 1), (0, 3, 0, 2), (0, 4, 1, 0), (2, 3, 0, 0), (2, 3, 0, 1),
                                           (2, 3, 0, 2)]
    for t, v in rows.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["AGPRs"] == 256 and v["Occupancy [waves/SIMD]"] == 1, (t, v)
