"""-m gpu: the multi-crop front end (acx_preprocess_crops) against Pillow, and the feature extractor (anomalyclip_amd/extract.py)
from frame folders to `.npy` files: against direct encoder calls, against the oracle on the Pillow-restated crops, through
FeatureStream into the head, and its resume behaviour."""
import dataclasses
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

import crops_restated as CR
from anomalyclip_amd import extract as X
from anomalyclip_amd import feature_index as FI
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd.components.anomaly_clip import AnomalyCLIP
from anomalyclip_amd.feature_stream import FeatureStream
from anomalyclip_amd.preprocess import CLIP_MEAN, CLIP_STD, default_scale_size, preprocess_crops, preprocess_frames
from oracle import anomalyclip_oracle as O
import recipes as R

DEV = "cuda"
TOL = 1e-4      # tests/test_gpu_model.py


def relerr(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def elem_ok(a, b):
    return R.elem_excess(a, b) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("geom", CR.GEOMETRIES + [(1080, 1920, 256, 224)])
@pytest.mark.parametrize("ncrops", [1, 5, 10])
def test_preprocess_crops_matches_pillow(geom, ncrops):
    """uint8 frames -> [F, ncrops, 3, C, C]: the 8-bit resample stages bit-exact with Pillow's scale + five_crop / ten_crop (the
    recovered uint8 image is equal everywhere), the float tail within test_frame_preprocessing_matches_pil's 2e-6.  240 x 320,
    odd margins, portrait, upscaling and the tiny geometry take the fused kernel; 336-pixel crops and the 1080p source (19 taps)
    the two-kernel route."""
    h, w, scale, crop = geom
    frames = CR.make_frames(h, w, 1 if h == 1080 else 2, seed=ncrops)
    ref = CR.pil_crops_float(frames.numpy(), scale, crop, ncrops)
    out = preprocess_crops(frames.to(DEV), crop, scale, ncrops)
    assert out.shape == (frames.shape[0], ncrops, 3, crop, crop) and out.dtype == torch.float32
    err = (out.cpu() - ref).abs().max().item()
    print(f"{geom} x {ncrops}: max |float difference| = {err:.3g}")
    m, s = torch.tensor(CLIP_MEAN).view(3, 1, 1), torch.tensor(CLIP_STD).view(3, 1, 1)
    assert torch.equal(((out.cpu() * s + m) * 255).round(), ((ref * s + m) * 255).round())
    assert err < 2e-6


@pytest.mark.parametrize("hw,size", [((240, 320), 224), ((360, 201), 224), ((480, 856), 336), ((97, 131), 32), ((224, 224), 224)])
def test_one_crop_at_scale_equals_preprocess_frames(hw, size):
    frames = CR.make_frames(hw[0], hw[1], 3, seed=7).to(DEV)
    a = preprocess_crops(frames, size, size, 1)
    assert a.shape == (3, 1, 3, size, size)
    assert torch.equal(a[:, 0], preprocess_frames(frames, size))
    assert torch.equal(preprocess_crops(frames, size), a)                      # scale_size defaults to crop_size for one crop


def test_default_scale_and_crop_order_on_the_device():
    """5 / 10 crops default to scale crop * 8 // 7; the first five of ten crops ARE the five crops; crop index minor to the frame"""
    frames = CR.make_frames(97, 131, 3, seed=3).to(DEV)
    five, ten = preprocess_crops(frames, 32, ncrops=5), preprocess_crops(frames, 32, ncrops=10)
    assert torch.equal(ten[:, :5], five) and torch.equal(five, preprocess_crops(frames, 32, default_scale_size(32, 5), 5))
    assert torch.equal(ten.view(30, 3, 32, 32)[1 * 10 + 7], ten[1, 7])
    one = preprocess_crops(frames[1:2], 32, 36, 10)
    assert torch.equal(one[0], ten[1])                                         # a frame's crops do not depend on its batch


# ---------------------------------------------------------------------------------------------------------------- the extractor
def _video(folder, T, hw, ext, seed):
    """T synthetic frames (moving gradient + noise + flat patches) as <folder>/{:06d}.<ext>"""
    os.makedirs(folder, exist_ok=True)
    rng = np.random.default_rng(seed)
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w]
    for t in range(T):
        a = np.stack([(xx * 3 + t * 5) % 256, (yy * 4 + t * 3) % 256, ((xx + yy) * 2 + t * 7) % 256], -1).astype(np.int64)
        a = np.clip(a + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8)
        a[: h // 4, : w // 4] = 255 if t % 2 else 0
        Image.fromarray(a).save(os.path.join(folder, f"{t:06d}.{ext}"), quality=90)


def _decoded(folder, T, ext):
    return np.stack([np.asarray(Image.open(os.path.join(folder, f"{t:06d}.{ext}")).convert("RGB")) for t in range(T)])


def _tiny_vit(seed=13, precision="f32"):
    enc = X.build_image_encoder("tiny", precision)
    sd = IW.init_vit_state_dict(IW.TINY, seed, prefix="")
    enc.load_state_dict(sd, strict=True)
    return enc.to(DEV).eval(), {"image_encoder." + k: v for k, v in sd.items()}


def _direct(enc, frames_u8, crop, ncrops, scale=None):
    """the same batch split as extract_video: max(1, chunk // ncrops) frames per preprocess_crops + encoder call"""
    nb = X.batch_frames(enc, ncrops)
    rows = []
    with torch.no_grad():
        for i in range(0, frames_u8.shape[0], nb):
            x = preprocess_crops(torch.from_numpy(frames_u8[i:i + nb]).to(DEV), crop, scale, ncrops)
            rows.append(enc(x.view(-1, 3, crop, crop)).cpu())
    return torch.cat(rows).numpy()


@pytest.mark.parametrize("ext,hw", [("png", (48, 64)), ("jpg", (64, 48)), ("jpg", (48, 64)), ("png", (64, 48))])
@pytest.mark.parametrize("ncrops", [1, 5, 10])
def test_extract_tiny_videos(tmp_path, ext, hw, ncrops):
    """three videos of 40 / 300 / 700 frames -> files [T * ncrops, 128] f32: bit-equal to encoding preprocess_crops of the same
    decoded frames at the same batch split, and within test_ncentroid_from_frames_tiny's 1e-5 of the oracle's ViT on the
    Pillow-restated crops"""
    enc, sd = _tiny_vit()
    root, out = str(tmp_path / "frames"), str(tmp_path / "feats")
    lens = {"a/v40": 40, "a/v300": 300, "b/v700": 700}
    for i, (v, T) in enumerate(lens.items()):
        _video(os.path.join(root, v), T, hw, ext, seed=i)
    anno = tmp_path / "anno.txt"
    anno.write_text("".join(f"{v} 0 {T - 1} 0\n" for v, T in lens.items()))
    counts = X.extract_dataset(enc, str(anno), root, out, ncrops=ncrops, template="{:06d}." + ext)
    assert counts == {"written": 3, "skipped": 0, "frames": 1040, "rows": 1040 * ncrops}
    scale = default_scale_size(32, ncrops)
    for v, T in lens.items():
        got = np.load(os.path.join(out, v + ".npy"), allow_pickle=False)
        assert got.shape == (T * ncrops, 128) and got.dtype == np.float32
        assert not os.path.exists(os.path.join(out, v + ".npy.tmp"))
        dec = _decoded(os.path.join(root, v), T, ext)
        assert np.array_equal(got, _direct(enc, dec, 32, ncrops))
        ref = O.vit_forward(sd, CR.pil_crops_float(dec, scale, 32, ncrops).view(-1, 3, 32, 32))
        e = relerr(got, ref)
        print(f"{v} {ext} {hw} x {ncrops}: relerr vs oracle on Pillow crops = {e:.3g}")
        assert e < 1e-5


def _big_encoder(arch, precision):
    geom = {"ViT-B/16": IW.VIT_B16, "RN50x4": IW.RN50X4}[arch]
    with torch.device(DEV):
        enc = X.build_image_encoder(arch, precision)
    init = IW.init_resnet_state_dict if geom.is_resnet else IW.init_vit_state_dict
    enc.load_state_dict(init(geom, 17, prefix=""), strict=True)
    return enc.eval()


@pytest.mark.parametrize("arch,precision,split_bound", [("ViT-B/16", "auto", 2e-6), ("ViT-B/16", "f32", 2e-6), ("RN50x4", "auto", 1e-5)])
def test_extract_full_size_encoders(tmp_path, arch, precision, split_bound):
    """24 frames of 240 x 320, 5 crops (ViT-B/16: 224 from 256, the fused kernel; RN50x4: 288 from 329, the two-kernel route):
    the file equals a direct encoder call at the same batch split bit for bit; a second split (8 frames = 40 rows per launch)
    agrees within the bound the launch-size tests hold that encoder to (test_vit_b16_golden / test_vit_b16_full_clip_properties:
    2e-6; test_resnet_full_launch_properties: 1e-5)."""
    enc = _big_encoder(arch, precision)
    C_ = enc.input_resolution
    root = str(tmp_path / "frames")
    _video(os.path.join(root, "v"), 24, (240, 320), "jpg", seed=5)
    dec = _decoded(os.path.join(root, "v"), 24, "jpg")
    r = X.extract_video(enc, X.FrameFolderReader(root, "v"), str(tmp_path / "one.npy"), ncrops=5)
    assert r == {"written": True, "frames": 24, "rows": 120}
    one = np.load(str(tmp_path / "one.npy"))
    assert one.shape == (120, enc.output_dim) and np.isfinite(one).all()
    assert np.array_equal(one, _direct(enc, dec, C_, 5))
    enc.chunk = 40
    assert X.batch_frames(enc, 5) == 8
    X.extract_video(enc, X.FrameFolderReader(root, "v"), str(tmp_path / "two.npy"), ncrops=5)
    two = np.load(str(tmp_path / "two.npy"))
    assert np.array_equal(two, _direct(enc, dec, C_, 5))
    e = relerr(two, one)
    print(f"{arch} {precision}: 8-frame launches vs one 24-frame launch: {e:.3g}")
    assert e < split_bound
    # pre-decoded frames (pinned memory) take the same path
    X.extract_video(enc, torch.from_numpy(dec).pin_memory(), str(tmp_path / "three.npy"), ncrops=5)
    assert np.array_equal(np.load(str(tmp_path / "three.npy")), two)


def test_resnet_in_training_mode_is_refused(tmp_path):
    enc = _big_encoder("RN50x4", "auto").train()
    with pytest.raises(ValueError, match="eval mode"):
        X.extract_video(enc, torch.zeros(2, 64, 64, 3, dtype=torch.uint8), str(tmp_path / "x.npy"), ncrops=1)


def test_round_trip_files_to_head(tmp_path, prompts_table):
    """frames -> 5-crop files -> FeatureStream(ncrops=5) -> net(..., test_mode) on a tiny-geometry net with XD_HEAD's crops,
    against the oracle's head on features the oracle's ViT computed from the Pillow-restated crops (test_gpu_model.py's bounds)"""
    hc = dataclasses.replace(IW.XD_HEAD, emb_size=64, heads=2, depth=1)
    assert hc.ncrops == 5
    toks = torch.tensor(prompts_table["xd"]["tokenized_prompts"], dtype=torch.int32)
    net = AnomalyCLIP(arch="tiny", labels_key="xd", emb_size=hc.emb_size, depth=hc.depth, heads=hc.heads, dim_heads=hc.dim_heads,
                      num_segments=32, seg_length=16, concat_features=hc.concat_features, normal_id=hc.normal_id, stride=1,
                      load_from_features=True, select_idx_dropout_topk=0.7, select_idx_dropout_bottomk=0.7, ncrops=hc.ncrops,
                      num_topk=3, num_bottomk=3, n_ctx=8, shared_context=False, ctx_init="")
    sd = IW.init_anomalyclip_state_dict(IW.TINY, hc, toks, 19)
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not missing and not unexpected
    net = net.to(DEV).eval()
    root, out = str(tmp_path / "frames"), str(tmp_path / "feats")
    lens = {"v300": 300, "v700": 700}
    for i, (v, T) in enumerate(lens.items()):
        _video(os.path.join(root, v), T, (48, 64), "jpg", seed=20 + i)
    counts = X.extract_dataset(net, None, root, out, ncrops=5)                 # the net's own image encoder; no annotation file
    assert counts["written"] == 2 and counts["rows"] == 5000
    paths = [os.path.join(out, v + ".npy") for v in lens]
    nc = torch.randn(128, generator=torch.Generator().manual_seed(4)) * 0.1
    for (feats, T_, S, path), (v, T) in zip(FeatureStream(paths, ncrops=5, device=torch.device(DEV)), lens.items()):
        assert T_ == T and feats.shape == (1, 5, 512 * S, 128)
        with torch.no_grad():
            sim, sc = net(feats, None, nc, S, True)
        dec = _decoded(os.path.join(root, v), T, "jpg")
        rows = O.vit_forward(sd, CR.pil_crops_float(dec, 36, 32, 5).view(-1, 3, 32, 32)).numpy()
        tile, S_ = FI.gather_test_features(rows, 32, 16, 1, ncrops=5)
        assert S_ == S
        rs, rc = O.anomaly_clip_forward_test(sd, hc, torch.from_numpy(np.ascontiguousarray(tile))[None], nc, toks.argmax(-1),
                                             IW.TINY.transformer_heads, S)
        print(f"{v}: similarity {relerr(sim, rs):.3g}, scores {relerr(sc, rc):.3g}")
        assert relerr(sim, rs) < TOL and relerr(sc, rc) < TOL
        assert elem_ok(sim, rs) and elem_ok(sc, rc)


def test_resume_skips_complete_files_and_rewrites_wrong_ones(tmp_path):
    enc, _ = _tiny_vit()
    root, out = str(tmp_path / "frames"), str(tmp_path / "feats")
    for i, (v, T) in enumerate((("x/a", 33), ("x/b", 20))):
        _video(os.path.join(root, v), T, (48, 64), "jpg", seed=30 + i)
    first = X.extract_dataset(enc, None, root, out, ncrops=5)
    assert first == {"written": 2, "skipped": 0, "frames": 53, "rows": 265}
    pa, pb = os.path.join(out, "x", "a.npy"), os.path.join(out, "x", "b.npy")
    keep = np.load(pa)
    os.utime(pa, ns=(10 ** 18, 10 ** 18))
    os.utime(pb, ns=(10 ** 18, 10 ** 18))
    open(pa + ".tmp", "wb").write(b"interrupted")                              # a stale .tmp beside a complete file
    again = X.extract_dataset(enc, None, root, out, ncrops=5)
    assert again == {"written": 0, "skipped": 2, "frames": 0, "rows": 0}
    assert os.stat(pa).st_mtime_ns == 10 ** 18 and os.stat(pb).st_mtime_ns == 10 ** 18
    np.save(pb, np.zeros((7, 128), np.float32))                                # a file cut short: another header shape
    os.utime(pb, ns=(10 ** 18, 10 ** 18))
    third = X.extract_dataset(enc, None, root, out, ncrops=5)
    assert third == {"written": 1, "skipped": 1, "frames": 20, "rows": 100}
    assert os.stat(pa).st_mtime_ns == 10 ** 18 and os.stat(pb).st_mtime_ns != 10 ** 18
    assert np.load(pb).shape == (100, 128)
    # other crop counts are other shapes: not complete; overwrite rewrites a complete file
    assert X.extract_dataset(enc, None, root, out, ncrops=10)["written"] == 2
    assert X.extract_dataset(enc, None, root, out, ncrops=10, overwrite=True)["written"] == 2
    assert np.load(pa).shape == (330, 128) and keep.shape == (165, 128)
    assert not os.path.exists(pb + ".tmp")


def test_command_line_end_to_end(tmp_path):
    """`python -m anomalyclip_amd.extract` in a child process: a Lightning-style checkpoint (`net.image_encoder.*`), a folder without
    annotations, 5 crops -> the same file as extract_dataset in this process; its counts as one JSON line"""
    import json
    import subprocess
    import sys
    enc, sd = _tiny_vit(seed=23)
    ckpt = str(tmp_path / "last.ckpt")
    torch.save({"state_dict": {"net." + k: v for k, v in sd.items()}, "epoch": 1}, ckpt)
    root = str(tmp_path / "frames")
    _video(os.path.join(root, "v"), 21, (48, 64), "jpg", seed=40)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "anomalyclip_amd.extract", "--arch", "tiny", "--weights", ckpt, "--frames-root", root,
           "--out-root", str(tmp_path / "cli"), "--ncrops", "5", "--precision", "f32"]
    r = subprocess.run(cmd, cwd=repo, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"written": 1, "skipped": 0, "frames": 21, "rows": 105}
    X.extract_dataset(enc, None, root, str(tmp_path / "here"), ncrops=5)
    assert np.array_equal(np.load(str(tmp_path / "cli" / "v.npy")), np.load(str(tmp_path / "here" / "v.npy")))
