"""Visualizer(entropy="gpu"): the qualitative videos with their frames Huffman-coded on the device are byte for byte the videos of
entropy="host" -- through Trainer.test in the frames mode, through the host fallback for a frame that passes its slot, and when
a clip is split into parts."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_frames_mode as FM                      # (names only: no test of those modules is collected again)
import test_gpu_visualizer as TV
import viz_ref as R
from anomalyclip_amd import ops
from anomalyclip_amd import visualizer as V
from anomalyclip_amd.datamodule import AnomalyCLIPDataModule
from anomalyclip_amd.trainer import Trainer

DEV = TV.DEV
e2e = TV.e2e                                           # the module's fixture: its two test videos have 21 and 19 frames


def trainer_test(root, frames, hp, entropy):
    base = root / f"entropy_{entropy}"
    mod, net = FM.build_module(False, base / "save", base / "logs")
    net.eval()
    dm = AnomalyCLIPDataModule(**hp, frames_root=frames, load_from_features=False, encoder=net, decode="gpu", visualize=True,
                               visualizer=dict(canvas=(320, 240), quality=90, batch=8, entropy=entropy))
    Trainer().test(mod, dm)
    torch.cuda.synchronize()
    return mod, base / "logs" / "train" / "runs" / "ckpt" / "qualitatives_var"


def test_trainer_test_writes_the_same_videos(e2e):
    """21 and 19 frames in batches of 8: the last batch of each video is partial"""
    root, frames, hp = e2e
    files = {}
    for entropy in ("host", "gpu"):
        mod, out_dir = trainer_test(root, frames, hp, entropy)
        viz = mod.visualizer
        assert viz.entropy == entropy and viz.frames_written == 40
        assert (viz._pool is None) == (entropy == "gpu")
        assert sorted(os.listdir(out_dir)) == ["t0.avi", "t1.avi"]
        files[entropy] = {f: (out_dir / f).read_bytes() for f in os.listdir(out_dir)}
        moved = viz.bytes_to_host
        viz.close()
        if entropy == "host":
            assert moved == 40 * 320 * 240 * 3
        else:                                          # the files' bytes and nothing else
            assert moved == sum(len(f) for data in files["gpu"].values() for f in R.walk_avi(data)["frames"])
    assert files["gpu"] == files["host"]
    assert [len(R.walk_avi(files["gpu"][f])["frames"]) for f in ("t0.avi", "t1.avi")] == [21, 19]


def render(frames, tmp, entropy, tag, cap=None, **kw):
    """the 21 frames of test/t0 with made-up scores through a Visualizer of its own -> {file name: bytes}, the Visualizer"""
    T, C1 = 21, 13
    rng = np.random.default_rng(5)
    scores = torch.from_numpy(rng.random(T).astype(np.float32))
    softmax = torch.softmax(torch.from_numpy(rng.normal(size=(T, C1)).astype(np.float32)), 1)
    labels = torch.tensor([FM.NORMAL_ID] * 8 + [3] * 13)
    viz = V.Visualizer(FM.NORMAL_ID, None, "{:06d}.jpg", str(tmp / tag), DEV, decode="gpu", canvas=(320, 240), quality=90, batch=8,
                       entropy=entropy, **kw)
    if cap is not None:
        viz.cap = cap
    viz.process_video(scores, None, softmax, labels, os.path.join(frames, "test", "t0"))
    torch.cuda.synchronize()
    viz.close()
    out = tmp / tag / "qualitatives_var"
    return {f: (out / f).read_bytes() for f in sorted(os.listdir(out))}, viz


def test_host_fallback_for_frames_that_pass_their_slot(e2e, tmp_path):
    """a per-frame slot of 1 KB holds none of the frames (1,800 blocks of 4 bits at least, and the header): every one goes through
    the host coder's retry"""
    root, frames, _ = e2e
    want, _ = render(frames, tmp_path, "host", "host")
    got, viz = render(frames, tmp_path, "gpu", "gpu_small", cap=1024)
    sizes = [len(f) for f in R.walk_avi(want["t0.avi"])["frames"]]
    assert len(sizes) == 21 and min(sizes) > 1024
    assert viz._dev["cap"] == 1024 and viz._pool is None
    assert viz.bytes_to_host == 21 * ops.jpeg_coef_elems(240, 320, 3, 2, 2) * 2       # the coefficients, as the host path copies them
    assert got == want
    # ... and a slot between the smallest and the largest file: some frames from the device, the others from the host
    cap = sorted(sizes)[10]
    mixed, viz = render(frames, tmp_path, "gpu", "gpu_mixed", cap=cap)
    assert mixed == want
    fit = [s for s in sizes if s <= cap]
    assert 0 < len(fit) < 21 and viz.bytes_to_host == sum(fit) + (21 - len(fit)) * 320 * 240 * 3


def test_split_into_parts(e2e, tmp_path):
    root, frames, _ = e2e
    want, _ = render(frames, tmp_path, "host", "host", max_file_bytes=60_000)
    got, _ = render(frames, tmp_path, "gpu", "gpu", max_file_bytes=60_000)
    assert len(want) >= 2 and list(want)[:2] == ["t0.avi", "t0.part1.avi"]
    assert got == want
    assert sum(len(R.walk_avi(d)["frames"]) for d in got.values()) == 21
