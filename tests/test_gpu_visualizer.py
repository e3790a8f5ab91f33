"""-m gpu: the qualitative videos.  The composed picture against a Pillow oracle bit for bit, the forward JPEG transform against
DESIGN.md's integer arithmetic restated in numpy (exactly) and against fp64 (within one), the files through the project's own device
decoder, their quality against Pillow's encoder, and `Trainer.test` with `visualize=True` end to end."""
import io
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw

pytestmark = pytest.mark.gpu

import viz_ref as R
from anomalyclip_amd import jpeg, ops
from anomalyclip_amd import visualizer as V
from anomalyclip_amd.datamodule import AnomalyCLIPDataModule
from anomalyclip_amd.trainer import Trainer, _to_device

DEV = torch.device("cuda", 0)
THR = 0.5
# Ours against Pillow's own encoder on the same canvas at the same quality ("Qualitative videos", holds the
# pairs): PSNR may be lower by at most PSNR_MARGIN_DB, the file larger by at most SIZE_MARGIN.  Both are the largest gap among the
# recorded pairs (the composed 1200 x 800 canvases and the photograph-like one, Q = 75 and 90), rounded up to the next 0.05 dB and
# the next 1 %: the largest PSNR gap was +0.003 dB (-> 0.05 dB); our file was smaller than Pillow's in every pair, the largest gap
# -0.16 % (-> 0 %).
PSNR_MARGIN_DB = 0.05
SIZE_MARGIN = 0.0


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C"))                                   # (a copy: Pillow's arrays are read-only)
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ====================================================================================================== composition
def probabilities(B, C1, PH, rng):
    """[B, C1] float32: 0, 1 and values whose p * PH + 0.5 lies within 1e-3 of an integer from below; the three largest of a row
    differ"""
    p = rng.random((B, C1)).astype(np.float32) * np.float32(0.9)
    for b in range(B):
        m = rng.permutation(np.arange(1, PH - 1))[:C1]                              # distinct: no two bars tie
        near = ((m + 0.5 - 5e-4) / PH).astype(np.float32)                         # p * PH + 0.5 = m + 1 - 5e-4
        pick = rng.random(C1) < 0.5
        p[b, pick] = near[pick]
        if C1 >= 3:
            p[b, rng.integers(0, C1)] = 0.0
            p[b, (b * 5 + 1) % C1] = 1.0
        else:
            p[b, 0] = (1.0, 0.0, near[0], 0.25)[b % 4]
        top = np.sort(p[b])[::-1][:3]
        assert len(set(top.tolist())) == len(top)                                   # no ties among the top three
    return p


def compose_case(canvas, source, C1, T, B, seed, static=None):
    rng = np.random.default_rng(seed)
    lay = V.layout(canvas, C1, source, T)
    PH = lay["bars_panel"][3] - lay["bars_panel"][1]
    if static is None:
        static = rng.integers(0, 256, (canvas[1], canvas[0], 3), dtype=np.uint8)    # random: a pixel drawn where none belongs shows
    frames = rng.integers(0, 256, (B, *source, 3), dtype=np.uint8)
    scores = np.array([0.2, THR, 0.9, np.nextafter(np.float32(THR), np.float32(0))], dtype=np.float32)[np.arange(B) % 4]
    p = probabilities(B, C1, PH, rng)
    idx = np.array(([0, T - 1] + list(rng.integers(0, T, size=B)))[:B], dtype=np.int32)
    got = ops.viz_compose(dev(static), dev(frames), dev(scores), dev(p), dev(idx), V.resize_tables(lay, DEV), V.geom_of(lay, THR))
    want = np.stack([R.compose_oracle(lay, static, frames[b], scores[b], p[b], int(idx[b]), THR) for b in range(B)])
    return lay, got, want


COMPOSE = [  # canvas, source (H, W), C1, T, B
    ((1200, 800), (240, 320), 13, 50, 4),      # 320x240: an upscale; scores below, at, above and just below the threshold
    ((1200, 800), (720, 1280), 64, 7, 3),      # 1280x720: a downscale whose filter support is above 2
    ((1200, 800), (320, 240), 1, 1, 1),        # 240x320: letterboxed the other way; C1 = 1, T = 1, B = 1
    ((320, 240), (29, 37), 13, 50, 4),         # 37x29: odd sizes, short table rows at the edges
    ((320, 240), (240, 320), 64, 50, 3),       # bars one pixel wide
    ((320, 240), (240, 320), 1, 3, 4),         # C1 = 1 with p = 1, 0, near an integer
]


@pytest.mark.parametrize("canvas,source,C1,T,B", COMPOSE)
def test_compose_equals_pillow_oracle(canvas, source, C1, T, B):
    lay, got, want = compose_case(canvas, source, C1, T, B, seed=C1 + T)
    f = lay["frame"]
    if source == (720, 1280):
        assert resample_support(source[1], f[2] - f[0]) > 2
    assert got.shape == want.shape and got.dtype == torch.uint8
    assert torch.equal(got.cpu(), torch.from_numpy(want))


def resample_support(in_size, out_size):
    return max(in_size / out_size, 1.0) * 2            # taps of the triangle filter: 2 * support


def test_compose_refusals():
    """C1 outside 1 .. 64 and a rectangle that touches the canvas edge are ACX_E_BADARG before any launch"""
    from anomalyclip_amd import _lib
    canvas, source = (320, 240), (48, 64)
    lay = V.layout(canvas, 13, source, 10)
    static = torch.full((240, 320, 3), 7, dtype=torch.uint8, device=DEV)
    args = (static, torch.zeros(2, 48, 64, 3, dtype=torch.uint8, device=DEV), torch.zeros(2, device=DEV), torch.zeros(2, 13, device=DEV),
            torch.zeros(2, dtype=torch.int32, device=DEV), V.resize_tables(lay, DEV))
    out = torch.full((2, 240, 320, 3), 9, dtype=torch.uint8, device=DEV)
    sp, pitch, bar_w = lay["score_panel"], lay["bar_pitch"], lay["bar_w"]
    for field, value in (("fx", 5), ("sy", 0), ("bx", 320 - 12 * pitch - bar_w), ("sx", 320 - (sp[2] - sp[0])), ("C1", 65)):
        g = V.geom_of(lay, THR)
        setattr(g, field, value)
        sm = torch.zeros(2, g.C1, device=DEV)
        with pytest.raises(_lib.AcxError, match="inside the canvas|C1"):
            ops.viz_compose(args[0], args[1], args[2], sm, args[4], args[5], g, out=out)
    torch.cuda.synchronize()
    assert bool((out == 9).all())                      # nothing was launched
    assert torch.equal(ops.viz_compose(*args, V.geom_of(lay, THR), out=out), out) and not bool((out == 9).all())


# ====================================================================================================== forward JPEG
def contents(H, W, seed):
    """[5, H, W, 3]: flat 0, flat 255, a full-scale checkerboard at pixel pitch, random bytes, a smooth ramp"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    check = (((yy + xx) & 1) * 255).astype(np.uint8)
    ramp = np.stack([xx * 255 // max(W - 1, 1), yy * 255 // max(H - 1, 1), (xx + yy) * 255 // max(W + H - 2, 1)], -1).astype(np.uint8)
    return np.stack([np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8), np.repeat(check[..., None], 3, -1),
                     rng.integers(0, 256, (H, W, 3), dtype=np.uint8), ramp])


def composed_canvases(B=2):
    """1200 x 800 canvases as the Visualizer composes them (its own static layer under the device's drawing)"""
    canvas, source, C1, T = (1200, 800), (240, 320), 13, 50
    lay = V.layout(canvas, C1, source, T)
    static = V.static_layer(lay, 0.5 + 0.4 * np.sin(np.arange(T) / 5.0), np.r_[np.full(20, 7), np.full(15, 3), np.full(15, 7)], 7,
                            [f"Class{k}" for k in range(C1)], "Arson011_x264")
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:240, 0:320]
    frames = np.stack([np.clip(np.stack([128 + 90 * np.sin(xx / (23.0 + b)) * np.cos(yy / 31.0), 128 + 80 * np.cos(xx / 41.0 + b),
                                         128 + 100 * np.sin((xx + yy) / 57.0)], -1) + rng.normal(0, 4, (240, 320, 3)), 0, 255)
                       for b in range(B)]).astype(np.uint8)
    scores = np.array([0.8, 0.3, 0.6, 0.1], np.float32)[:B]
    p = rng.dirichlet(np.ones(C1), size=B).astype(np.float32)
    idx = np.array([10, 40, 0, 49], np.int32)[:B]
    got = ops.viz_compose(dev(static), dev(frames), dev(scores), dev(p), dev(idx), V.resize_tables(lay, DEV), V.geom_of(lay, THR))
    return got


def photo_canvas():
    """a photograph-like smooth field with text over it, 1200 x 800"""
    yy, xx = np.mgrid[0:800, 0:1200]
    rng = np.random.default_rng(11)
    a = np.stack([128 + 100 * np.sin(xx / 97.0) * np.cos(yy / 71.0), 128 + 90 * np.cos((xx - yy) / 133.0), 128 + 110 * np.sin(yy / 53.0 + xx / 211.0)], -1)
    img = Image.fromarray(np.clip(a + rng.normal(0, 3, a.shape), 0, 255).astype(np.uint8))
    d = ImageDraw.Draw(img)
    for k in range(12):
        d.text((40 + 60 * k, 30 + 60 * k), "qualitative video: P(c|A), p(A), Frame Number", fill=(255, 255, 255) if k & 1 else (0, 0, 0))
    return np.asarray(img)


@pytest.fixture(scope="module")
def forward_sets():
    """[(name, canvases uint8 [B, Hc, Wc, 3] on the host)], computed once"""
    return [("16x16", contents(16, 16, 1)), ("48x32", contents(32, 48, 2)), ("composed 1200x800", composed_canvases(1).cpu().numpy())]


@pytest.mark.parametrize("quality", [50, 90, 100])
def test_forward_equals_the_stated_arithmetic_and_fp64_within_one(forward_sets, quality):
    qt = V.quant_tables(quality)
    qd = dev(qt.view(np.int16))
    differ = total = 0
    for name, canv in forward_sets:
        got = ops.jpeg_forward(dev(canv), qd).cpu().numpy()
        assert got.shape == (canv.shape[0], canv.shape[1] * canv.shape[2] * 3 // 2) and got.dtype == np.int16
        for b in range(canv.shape[0]):
            assert np.array_equal(got[b], R.forward_restated(canv[b], qt)), (name, b, quality)       # exact: the stated integers
            ref = R.forward_fp64(canv[b], qt)
            err = np.abs(got[b].astype(np.float64) - ref)
            assert err.max() <= 1, (name, b, quality, err.max())                                     # derived: see DESIGN.md
            differ += int((err != 0).sum())
            total += err.size
    print(f"quality {quality}: {differ} of {total} coefficients differ from fp64 ({100.0 * differ / total:.4f} %)")


def test_forward_refusals():
    from anomalyclip_amd import _lib
    qd = dev(V.quant_tables(90).view(np.int16))
    for shape in ((1, 24, 32, 3), (1, 32, 40, 3)):
        with pytest.raises(_lib.AcxError, match="multiples of 16"):
            ops.jpeg_forward(torch.zeros(shape, dtype=torch.uint8, device=DEV), qd)


def encode_file(coef_row: np.ndarray, qt, H, W) -> bytes:
    buf = np.empty(ops.jpeg_encode_bound(H, W), np.uint8)
    n = ops.jpeg_entropy_encode(np.ascontiguousarray(coef_row), qt, H, W, buf)
    assert n > 0
    return buf[:n].tobytes()


def test_round_trip_through_the_device_decoder(tmp_path):
    """acx_jpeg_forward -> acx_jpeg_entropy_encode -> decode="gpu": bit for bit Pillow's convert("RGB") of the same files, all of
    them on the device path (no Pillow fallback)"""
    lay, got, _ = compose_case((320, 240), (48, 64), 13, 20, 3, seed=9, static=V.static_layer(
        V.layout((320, 240), 13, (48, 64), 20), np.linspace(0, 1, 20), np.r_[np.full(8, 7), np.full(12, 2)], 7, None, "t0"))
    qt = V.quant_tables(90)
    coef = ops.jpeg_forward(got, dev(qt.view(np.int16))).cpu().numpy()
    folder = tmp_path / "v"
    folder.mkdir()
    files = [encode_file(coef[b], qt, 240, 320) for b in range(3)]
    for b, data in enumerate(files):
        (folder / f"{b:06d}.jpg").write_bytes(data)
    reader = jpeg.make_reader("gpu", str(tmp_path), "v", 0, 2)
    out = torch.cat([x.clone() for _, x in reader.batches(2)])
    assert reader.fallbacks == 0 and reader.geometry == (240, 320, 3, 2, 2)
    want = np.stack([R.pillow_decode(d) for d in files])
    assert torch.equal(out.cpu(), torch.from_numpy(want))


def quality_pairs(canvas: np.ndarray, quality: int):
    """((PSNR ours, PSNR Pillow's), (bytes ours, bytes Pillow's)) of one canvas"""
    Hc, Wc, _ = canvas.shape
    qt = V.quant_tables(quality)
    coef = ops.jpeg_forward(dev(canvas[None]), dev(qt.view(np.int16))).cpu().numpy()[0]
    ours = encode_file(coef, qt, Hc, Wc)
    buf = io.BytesIO()
    Image.fromarray(canvas).save(buf, "JPEG", quality=quality, subsampling=2)
    theirs = buf.getvalue()
    return (R.psnr(R.pillow_decode(ours), canvas), R.psnr(R.pillow_decode(theirs), canvas)), (len(ours), len(theirs))


@pytest.mark.parametrize("quality", [75, 90])
def test_picture_quality_against_pillows_encoder(quality):
    """Pillow is the yardstick: PSNR of (Pillow-decoded our file) against the canvas may fall short of PSNR of (Pillow-decoded
    Image.save(quality=Q, subsampling=2)) by at most PSNR_MARGIN_DB = 0.05 dB, and our file may be larger than Pillow's by at most
    SIZE_MARGIN = 0 % (it was smaller in every recorded pair: the largest gap, -0.16 %, rounds up to 0).  Both margins are the largest gap among the pairs recorded in DESIGN.md section 4 ("Qualitative videos":
    two composed 1200 x 800 canvases and the photograph-like canvas, Q = 75 and 90), rounded up to the next 0.05 dB and the next
    1 %.  The differences come from the chroma filter and from DCT rounding only; a larger gap means a wrong table or zigzag."""
    canv = [("composed 0", None), ("composed 1", None), ("photo", photo_canvas())]
    comp = composed_canvases(2).cpu().numpy()
    canv[0], canv[1] = ("composed 0", comp[0]), ("composed 1", comp[1])
    for name, c in canv:
        (po, pp), (so, sp_) = quality_pairs(c, quality)
        print(f"Q={quality} {name}: PSNR ours {po:.3f} dB, Pillow {pp:.3f} dB (gap {pp - po:+.3f}); bytes ours {so}, Pillow {sp_} "
              f"({100.0 * (so - sp_) / sp_:+.2f} %)")
        assert po >= pp - PSNR_MARGIN_DB, (name, po, pp)
        assert so <= sp_ * (1 + SIZE_MARGIN), (name, so, sp_)


# ====================================================================================================== end to end
import test_gpu_frames_mode as FM                      # the tiny-geometry module and its helpers (names only: no test is re-collected)

NAMES = ["Class0", "Class1", "Class2", "Class3", "Class4", "Class5", "Class6", "Normal", "Class8", "Class9", "Class10", "RoadAccidents",
         "Class12", "Class13"]
VIDEOS = {"normal": [("normal/n0", 20, FM.NORMAL_ID)], "anomaly": [("anomaly/a0", 20, 3)], "test": [("test/t0", 21, 3), ("test/t1", 19, FM.NORMAL_ID)]}
CANVAS, QUALITY = (320, 240), 90


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    root = tmp_path_factory.mktemp("visualize")
    frames = str(root / "frames")
    lists = {}
    for k, (kind, vids) in enumerate(VIDEOS.items()):
        lists[kind] = str(root / f"{kind}.txt")
        with open(lists[kind], "w") as fh:
            for i, (v, n, lab) in enumerate(vids):
                FM._video(os.path.join(frames, v), n, (48, 64), "jpg", seed=100 + 10 * k + i)
                fh.write(f"{v} 0 {n - 1} {lab}\n")
    with open(root / "temporal.txt", "w") as fh:
        fh.write("t0.mp4 Arson 5 12 -1 -1\nt1.mp4 Normal -1 -1 -1 -1\n")          # one anomalous run
    with open(root / "labels.csv", "w") as fh:
        fh.write("id,name\n" + "".join(f"{i},{n}\n" for i, n in enumerate(NAMES)))
    hp = dict(annotation_file_normal=lists["normal"], annotation_file_anomaly=lists["anomaly"], annotation_file_test=lists["test"],
              annotation_file_temporal_test=str(root / "temporal.txt"), labels_file=str(root / "labels.csv"), normal_id=FM.NORMAL_ID,
              num_classes=FM.NUM_CLASSES, num_segments=FM.HEAD.num_segments, seg_length=FM.HEAD.seg_length, batch_size=2, device=DEV)
    return root, frames, hp


def run_test(root, frames, hp, mode, visualize, tag):
    """Trainer.test of a fresh tiny module -> (module, datamodule, returned metrics, per-video outputs, base directory)"""
    base = root / tag
    mod, net = FM.build_module(mode == "features", base / "save", base / "logs")
    net.eval()
    extra = dict(visualize=True, visualizer=dict(canvas=CANVAS, quality=QUALITY, batch=8)) if visualize else {}
    if mode == "features":
        feats = FM.extracted(root, frames, hp, net, 1, "viz")
        if visualize:
            extra["visualizer"]["frames_root"] = frames
        dm = AnomalyCLIPDataModule(**hp, frames_root=feats, **extra)
    else:
        dm = AnomalyCLIPDataModule(**hp, frames_root=frames, load_from_features=False, encoder=net, decode="gpu", **extra)
    seen = []
    real = mod.test_epoch_end
    mod.test_epoch_end = lambda outputs: (seen.append(outputs), real(outputs))[1]
    metrics = Trainer().test(mod, dm)
    torch.cuda.synchronize()
    return mod, dm, metrics, seen[0], base


@pytest.mark.parametrize("mode", ["features", "frames"])
def test_trainer_test_writes_the_videos(e2e, mode):
    root, frames, hp = e2e
    mod, dm, metrics, outputs, base = run_test(root, frames, hp, mode, True, f"{mode}_viz")
    assert mod.visualizer is not None and mod.visualizer.decode == ("gpu" if mode == "frames" else "pil")
    plain, _, plain_metrics, plain_outputs, plain_base = run_test(root, frames, hp, mode, False, f"{mode}_plain")
    assert plain.visualizer is None and not (plain_base / "logs" / "train" / "runs" / "ckpt" / "qualitatives_var").exists()
    # nothing the metrics see changes
    assert metrics and json.dumps(metrics, sort_keys=True) == json.dumps(plain_metrics, sort_keys=True)
    rel = "logs/eval/runs/ckpt/metrics.json"
    assert (base / rel).read_text() == (plain_base / rel).read_text()
    for a, b in zip(outputs, plain_outputs):
        assert all(torch.equal(a[k], b[k]) for k in ("abnormal_scores", "labels", "class_probs"))
    out_dir = base / "logs" / "train" / "runs" / "ckpt" / "qualitatives_var"
    assert sorted(os.listdir(out_dir)) == ["t0.avi", "t1.avi"]
    names = V.read_class_names(hp["labels_file"])
    assert len(names) == 13 and "Normal" not in names and "RoadAcc." in names
    qt = V.quant_tables(QUALITY)
    for (video, n, _), batch, o in zip(VIDEOS["test"], dm.test_dataloader(), outputs):
        name = video.split("/")[1]
        a = R.walk_avi((out_dir / f"{name}.avi").read_bytes())
        labels = o["labels"]
        assert len(a["frames"]) == a["avih_frames"] == labels.shape[0] == n and (a["width"], a["height"]) == CANVAS
        scores, lab, probs, softmax = mod._score_video(_to_device(batch, DEV), with_softmax=True)
        assert torch.equal(scores, o["abnormal_scores"]) and softmax.shape == (n, 13)
        lay = V.layout(CANVAS, 13, (48, 64), n)
        static = V.static_layer(lay, scores.cpu().numpy(), lab.cpu().numpy(), FM.NORMAL_ID, names, name)
        if name == "t0":
            assert set(lab.cpu().tolist()) == {3, FM.NORMAL_ID}
        for i in (0, n // 2, n - 1):
            frame = np.asarray(Image.open(os.path.join(frames, video, f"{i:06d}.jpg")).convert("RGB"))
            want = R.compose_oracle(lay, static, frame, float(scores[i]), softmax[i].cpu().numpy(), i, THR)
            got = R.pillow_decode(a["frames"][i])
            buf = io.BytesIO()
            Image.fromarray(want).save(buf, "JPEG", quality=QUALITY, subsampling=2)
            ours, theirs = R.psnr(got, want), R.psnr(R.pillow_decode(buf.getvalue()), want)
            print(f"{mode} {name} frame {i}: PSNR {ours:.3f} dB, Pillow's encoder {theirs:.3f} dB")
            assert ours >= theirs - PSNR_MARGIN_DB, (name, i, ours, theirs)
    # a second test call leaves the files alone
    before = {f: os.stat(out_dir / f).st_mtime_ns for f in os.listdir(out_dir)}
    Trainer().test(mod, dm)
    assert {f: os.stat(out_dir / f).st_mtime_ns for f in os.listdir(out_dir)} == before
    mod.visualizer.close()
