"""-m gpu: training, validation and test from frame folders (`data.load_from_features: false`).  The test-mode tile kernel
(acx_tile_videos, a pure copy) against feature_index.gather_test_features in numpy, a bank filled by the encoder against the files
`extract` writes, and the datamodule / trainer in frames mode against the same run over those files.  Every comparison is bit for
bit: the kernel copies, and both sinks of the encode loop make the same launches."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib, ops
from anomalyclip_amd import extract as X
from anomalyclip_amd import feature_index as FI
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd.anomaly_clip_module import AnomalyCLIPModule
from anomalyclip_amd.components.anomaly_clip import AnomalyCLIP
from anomalyclip_amd.components.loss import ComputeLoss
from anomalyclip_amd.datamodule import AnomalyCLIPDataModule, ResidentTestLoader, StreamedTestLoader, read_annotation_file
from anomalyclip_amd.feature_bank import BankTile, FeatureBank
from anomalyclip_amd.trainer import Trainer
from test_gpu_extract import _tiny_vit, _video
from test_gpu_feature_bank import device_tables, i32
from test_gpu_head_grid import HC, _toks

DEV = torch.device("cuda", 0)
GRIDS = [(32, 16), (4, 2)]


# ====================================================================================================== the kernel
def tiles_reference(files, ncrops, vids, N, L, stride):
    """the tensor forward_test_many takes: the reference's test-mode tile of every video (crop-major), video after video"""
    tiles = [FI.gather_test_features(files[v], N, L, stride, ncrops) for v in vids]
    return np.concatenate([t.reshape(-1, t.shape[-1]) for t, _ in tiles]), [S for _, S in tiles]


def make_files(T, ncrops, D, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((t * ncrops, D)).astype(np.float32) for t in T]


@pytest.mark.parametrize("N,L", GRIDS)
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("ncrops", [1, 5])
@pytest.mark.parametrize("D", [64, 512, 640])
def test_tile_videos_mixed_group(D, ncrops, stride, N, L):
    """one group of three videos of 5, 513 and 1025 frames: a video shorter than a segment row, one frame past a 512-frame tile,
    one past two; then the same videos in another order with one of them twice"""
    T = [5, 513, 1025]
    files = make_files(T, ncrops, D, D + ncrops)
    bank, row_off = device_tables(files)
    for vids in ([0, 1, 2], [2, 0, 2, 1]):
        want, S = tiles_reference(files, ncrops, vids, N, L, stride)
        assert S == [-(-T[v] // (N * L * stride)) for v in vids]
        out = ops.tile_videos(bank, row_off, i32(T), vids, S, N, L, stride, ncrops)
        assert out.shape == want.shape and out.dtype == torch.float32 and out.is_contiguous()
        assert np.array_equal(out.cpu().numpy(), want), vids


@pytest.mark.parametrize("N,L", GRIDS)
@pytest.mark.parametrize("ncrops,stride", [(1, 1), (5, 3)])
def test_tile_videos_single_video_equals_sample_segments(N, L, ncrops, stride):
    """V = 1 is what acx_sample_segments gives for B = 1, N * S segments and the test-mode starts k * L * stride"""
    T = [37, 700]
    files = make_files(T, ncrops, 128, 3)
    bank, row_off = device_tables(files)
    for v in (0, 1):
        starts, S = FI.test_start_indices(T[v], N, L, stride)
        assert np.array_equal(starts, np.arange(N * S) * L * stride)
        want = ops.sample_segments(bank, row_off, i32(T), i32([v]), i32(starts), N * S, L, stride, ncrops)
        got = ops.tile_videos(bank, row_off, i32(T), [v], [S], N, L, stride, ncrops)
        assert torch.equal(got.view(want.shape), want)
        # into a caller's buffer
        buf = torch.full_like(got, -1.0)
        assert ops.tile_videos(bank, row_off, i32(T), [v], [S], N, L, stride, ncrops, out=buf) is buf and torch.equal(buf, got)


@pytest.mark.parametrize("ncrops,stride", [(1, 1), (5, 1), (1, 3)])
def test_tile_videos_shorter_than_one_segment(ncrops, stride):
    """T = 1 and T = 15 on the 32 x 16 grid: a 512-row tile wraps around the video 512 and 35 times"""
    T = [1, 15]
    files = make_files(T, ncrops, 64, 9)
    bank, row_off = device_tables(files)
    want, S = tiles_reference(files, ncrops, [0, 1], 32, 16, stride)
    assert S == [1, 1] and want.shape == (2 * ncrops * 512, 64)
    out = ops.tile_videos(bank, row_off, i32(T), [0, 1], S, 32, 16, stride, ncrops)
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(want[:512], np.repeat(files[0][:1], 512, 0))


def test_tile_videos_entry_point_checks():
    """V = 0 is ACX_OK; D % 4 != 0 and a misaligned out are ACX_E_BADARG with a message; none of them launches: the sentinel in
    `out` survives"""
    files = make_files([4], 1, 8, 1)
    bank, row_off = device_tables(files)
    frames, vid, rows, blk = i32([4]), i32([0]), i32([4]), i32([0])
    out_off = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = torch.full((8, 8), -7.0, device=DEV)
    fn, h, st = _lib.lib().acx_tile_videos, ops._h(bank), ops._stream()
    p = [t.data_ptr() for t in (bank, row_off, frames, vid, out_off, rows, blk, out)]
    assert fn(h, *p, 0, 4, 2, 2, 1, 1, 8, st) == 0                               # V == 0
    assert fn(h, *p, 1, 4, 2, 2, 1, 1, 6, st) == -1 and b"D % 4" in _lib.lib().acx_last_error(h)
    assert fn(h, *p[:7], out.data_ptr() + 4, 1, 4, 2, 2, 1, 1, 8, st) == -1 and b"aligned" in _lib.lib().acx_last_error(h)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert ops.tile_videos(bank, row_off, frames, [], [], 2, 2, 1, 1).shape == (0, 8)
    with pytest.raises(_lib.AcxError, match="acx_tile_videos"):
        ops.tile_videos(torch.ones(4, 6, device=DEV), row_off, frames, [0], [1], 2, 2, 1, 1)
    with pytest.raises(ValueError, match="tile_videos"):
        ops.tile_videos(bank, row_off, frames, [1], [1], 2, 2, 1, 1)             # a video index outside the bank
    assert fn(h, *p, 1, 4, 2, 2, 1, 1, 8, st) == 0                               # and the valid call copies
    assert np.array_equal(out[:4].cpu().numpy(), files[0]) and bool((out[4:] == -7.0).all())


def test_tile_videos_past_2_31_floats():
    """a bank of 2^31 + 40 * 512 floats (8.6 GB, never filled): its last 40 rows are one video, which lies past the boundary as a
    whole; it is tiled twice in one group and compared with the formula on those 40 rows.  Offsets must be 64-bit."""
    D, T = 512, 40
    rows = (1 << 31) // D + T
    bank = torch.empty(rows, D, dtype=torch.float32, device=DEV)
    assert bank.numel() > 1 << 31 and (rows - T) * D >= 1 << 31
    video = np.random.default_rng(0).standard_normal((T, D)).astype(np.float32)
    bank[rows - T:].copy_(torch.from_numpy(video))
    row_off = torch.tensor([0, rows - T], dtype=torch.int64, device=DEV)
    want, S = tiles_reference([None, video], 1, [1, 1], 4, 4, 1)
    assert S == [3, 3]
    out = ops.tile_videos(bank, row_off, i32([7, T]), [1, 1], S, 4, 4, 1, 1)
    assert np.array_equal(out.cpu().numpy(), want)
    del bank, out
    torch.cuda.empty_cache()


# ====================================================================================================== frame folders
NORMAL_ID, NUM_CLASSES = 7, 14
HEAD = HC(4, 2, 64, 2)
# (folder, frames in the folder, start_frame, end_frame, label): one row starts past frame 0 and ends before the folder does
NORMAL = [("normal/n0", 33, 0, 32, NORMAL_ID), ("normal/n1", 60, 10, 49, NORMAL_ID), ("normal/n2", 20, 0, 19, NORMAL_ID)]
ANOMALY = [("anomaly/a0", 70, 0, 69, 3), ("anomaly/a1", 25, 0, 24, 11), ("anomaly/a2", 47, 0, 46, 1)]
TEST = [("test/t0", 50, 0, 49, 3), ("test/t1", 29, 0, 28, NORMAL_ID)]


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """JPEG folders of 48 x 64 frames and the reference's list files -> (root, datamodule hyper-parameters without the mode)"""
    root = tmp_path_factory.mktemp("frames_mode")
    frames = str(root / "frames")
    lists = {}
    for k, (kind, vids) in enumerate((("normal", NORMAL), ("anomaly", ANOMALY), ("test", TEST))):
        lists[kind] = str(root / f"{kind}.txt")
        with open(lists[kind], "w") as fh:
            for i, (v, n, a, b, lab) in enumerate(vids):
                _video(os.path.join(frames, v), n, (48, 64), "jpg", seed=10 * k + i)
                fh.write(f"{v} {a} {b} {lab}\n")
    with open(root / "temporal.txt", "w") as fh:
        fh.write("t0.mp4 Arson 12 30 -1 -1\nt1.mp4 Normal -1 -1 -1 -1\n")
    hp = dict(annotation_file_normal=lists["normal"], annotation_file_anomaly=lists["anomaly"], annotation_file_test=lists["test"],
              annotation_file_temporal_test=str(root / "temporal.txt"), labels_file=None, normal_id=NORMAL_ID, num_classes=NUM_CLASSES,
              num_segments=HEAD.num_segments, seg_length=HEAD.seg_length, batch_size=2, device=DEV)
    return root, frames, hp


def build_net(load_from_features, ncrops=1, seed=31):
    """the tiny CLIP geometry under the 4 x 2 head (test_gpu_head_grid.build_grid_net, with the mode flag the reference's YAML ties
    to the data key)"""
    hc, toks = HEAD, _toks()
    net = AnomalyCLIP(arch="tiny", labels_key="ucf", emb_size=hc.emb_size, depth=hc.depth, heads=hc.heads, dim_heads=hc.dim_heads,
                      num_segments=hc.num_segments, seg_length=hc.seg_length, concat_features=hc.concat_features,
                      normal_id=hc.normal_id, stride=1, load_from_features=load_from_features, select_idx_dropout_topk=0.7,
                      select_idx_dropout_bottomk=0.7, ncrops=ncrops, num_topk=hc.num_topk, num_bottomk=hc.num_bottomk, n_ctx=8,
                      shared_context=False, ctx_init="")
    missing, unexpected = net.load_state_dict(IW.init_anomalyclip_state_dict(IW.TINY, hc, toks, seed), strict=False)
    assert not missing and not unexpected
    return net.to(DEV)


def build_module(load_from_features, save_dir, logs_root):
    net = build_net(load_from_features)
    hc = HEAD
    crit = ComputeLoss(hc.normal_id, hc.num_topk, 1.0, 1.0, 1.0, 1.0, 1.0, 8e-4, 8e-3, hc.seg_length, hc.num_segments)
    mod = AnomalyCLIPModule(net, None, None, crit, num_classes=NUM_CLASSES, solver={"lr": 1e-3}, save_dir=str(save_dir),
                            logs_root=str(logs_root)).to(DEV)
    return mod, net


def extracted(root, frames, hp, encoder, ncrops, tag):
    """the feature files `extract` writes for the three lists with `encoder` -> the root the features-mode datamodule reads"""
    out = str(root / f"features_{tag}_{ncrops}")
    for kind in ("normal", "anomaly", "test"):
        X.extract_dataset(encoder, hp[f"annotation_file_{kind}"], frames, out, ncrops=ncrops)
    return out


@pytest.fixture(scope="module")
def vit_files(folders):
    """test_gpu_extract's tiny ViT and the files it extracts, per crop count"""
    root, frames, hp = folders
    enc, _ = _tiny_vit()
    done = {}

    def get(ncrops):
        if ncrops not in done:
            done[ncrops] = extracted(root, frames, hp, enc, ncrops, "vit")
        return enc, done[ncrops]
    return get


@pytest.mark.parametrize("ncrops", [1, 5])
def test_bank_from_frames_equals_the_extracted_files(folders, vit_files, ncrops):
    root, frames, hp = folders
    enc, feats = vit_files(ncrops)
    recs = read_annotation_file(hp["annotation_file_normal"], feats) + read_annotation_file(hp["annotation_file_anomaly"], feats)
    lines = []
    bank = FeatureBank.from_frames(enc, recs, frames, "{:06d}.jpg", ncrops, log=lines.append)
    files = [np.load(r.path) for r in recs]
    assert [f.shape[0] for f in files] == [(b - a + 1) * ncrops for _, _, a, b, _ in NORMAL + ANOMALY]
    assert bank.bank.shape == (sum(f.shape[0] for f in files), 128) and bank.D == 128 and bank.device == DEV and len(bank) == 6
    assert np.array_equal(bank.bank.cpu().numpy(), np.concatenate(files))
    assert bank.num_frames == bank.file_frames == bank.frames.tolist() == [r.num_frames for r in recs]
    assert bank.row_off.tolist() == bank.offsets[:-1].tolist() and bank.labels.tolist() == [r.label for r in recs]
    assert bank.paths == [os.path.join(frames, v) for v, *_ in NORMAL + ANOMALY] and len(lines) == 6
    for v, f in enumerate(files):
        assert np.array_equal(bank.video(v).cpu().numpy(), f)
    # the same bank as the one loaded from the files
    again = FeatureBank([r.path for r in recs], [r.num_frames for r in recs], [r.label for r in recs], ncrops, DEV)
    assert torch.equal(again.bank, bank.bank) and torch.equal(again.row_off, bank.row_off) and torch.equal(again.frames, bank.frames)


def test_bank_from_frames_refusals(folders):
    root, frames, hp = folders
    enc, _ = _tiny_vit()
    recs = read_annotation_file(hp["annotation_file_test"], frames)
    with pytest.raises(ValueError, match=r"need \d+ bytes.*1024 bytes.*anomalyclip_amd\.extract"):
        FeatureBank.from_frames(enc, recs, frames, max_bytes=1024)
    recs[1].end_frame = 29                                       # test/t1 holds frames 0 ... 28
    with pytest.raises(FileNotFoundError, match=r"test/t1.*000029\.jpg"):
        FeatureBank.from_frames(enc, recs, frames)


def test_training_batches_equal_features_mode(folders, vit_files):
    """two epochs of both train loaders under the same seeds: frames mode against the features-mode datamodule over the extracted
    files"""
    root, frames, hp = folders
    enc, feats = vit_files(1)
    streams = []
    for kw in (dict(frames_root=frames, load_from_features=False, encoder=enc), dict(frames_root=feats)):
        torch.manual_seed(5)
        np.random.seed(6)
        dm = AnomalyCLIPDataModule(**hp, **kw)
        dm.setup("fit")
        got = []
        for _ in range(2):
            loaders = dm.train_dataloader()
            assert len(loaders) == 2 and all(len(l) == 3 for l in loaders)
            for (nf, nl), (af, al) in zip(*loaders):
                assert nf.shape == af.shape == (1, 1, 8, 128) and nf.device == DEV
                got.append((nf.clone(), nl.clone(), af.clone(), al.clone()))
        streams.append(got)
        assert dm.yields_features and [v.shape[0] for v in dm.resident_normal_videos()] == [33, 40, 20]
    assert len(streams[0]) == len(streams[1]) == 6
    for a, b in zip(*streams):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert len({float(a[0].sum()) for a in streams[0]}) > 1


@pytest.mark.parametrize("ncrops", [1, 5])
def test_test_tiles_equal_features_mode(folders, vit_files, ncrops):
    root, frames, hp = folders
    enc, feats = vit_files(ncrops)
    dm = AnomalyCLIPDataModule(**hp, frames_root=frames, load_from_features=False, encoder=enc, ncrops=ncrops)
    dm.setup("test")
    assert dm.bank is None                                        # evaluation encodes no training bank
    loader = dm.test_dataloader()
    assert isinstance(loader, ResidentTestLoader) and len(loader) == 2 and dm.val_dataloader().bank is loader.bank
    ref = AnomalyCLIPDataModule(**hp, frames_root=feats, ncrops=ncrops).test_dataloader()
    assert isinstance(ref, StreamedTestLoader)
    n = 0
    for (tile, lab, label, S, path), (rf, rlab, rlabel, rS, rpath), (v, _, a, b, _) in zip(loader, ref, TEST):
        assert isinstance(tile, BankTile) and tuple(tile.shape) == tuple(rf.shape) == (1, ncrops, 8 * int(rS), 128)
        assert torch.equal(tile.to(DEV), rf) and torch.equal(lab, rlab) and torch.equal(label, rlabel) and torch.equal(S, rS)
        assert lab.shape == (1, b - a + 1) and path == [os.path.join(frames, v)] and rpath == [os.path.join(feats, v) + ".npy"]
        n += 1
    assert n == 2 and set(loader.frame_labels(0, 50).tolist()) == {3, NORMAL_ID}
    # the normal list in test mode, without a fit bank: a bank of its own, every frame normal_id
    normal = list(dm.train_dataloader_test_mode())
    want = list(AnomalyCLIPDataModule(**hp, frames_root=feats, ncrops=ncrops).train_dataloader_test_mode())
    assert len(normal) == len(want) == 3 and dm.bank is None
    for (tile, lab, *_), (rf, rlab, *_) in zip(normal, want):
        assert torch.equal(tile.to(DEV), rf) and torch.equal(lab, rlab)


# ====================================================================================================== whole runs
def run(folders, mode, tag, max_epochs=2, ckpt_path=None, test=True, seeds=(77, 78)):
    """Trainer.fit (validation after every epoch, last.ckpt) and Trainer.test of a fresh module in `mode`; the net is built with
    the mode's own load_from_features.  Features mode reads the files that the same net's encoder extracted."""
    root, frames, hp = folders
    base = root / tag
    mod, net = build_module(mode == "features", base / "save", base / "logs")
    if mode == "features":
        dm = AnomalyCLIPDataModule(**hp, frames_root=extracted(root, frames, hp, net.eval(), 1, "net"))
    else:
        dm = AnomalyCLIPDataModule(**hp, frames_root=frames, load_from_features=False, encoder=net)
    net.train()
    torch.manual_seed(seeds[0])
    np.random.seed(seeds[1])
    Trainer(max_epochs=max_epochs, default_root_dir=str(base)).fit(mod, dm, ckpt_path=ckpt_path)
    ckpt = str(base / "checkpoints" / "last.ckpt")
    metrics = Trainer().test(mod, dm, ckpt_path=ckpt) if test else None
    torch.cuda.synchronize()
    weights = {n: p.detach().clone() for n, p in net.named_parameters()}
    weights.update({"buffer." + n: b.detach().clone() for n, b in net.selector_model.named_buffers()})
    return dict(mod=mod, dm=dm, base=base, ckpt=ckpt, weights=weights, metrics=metrics)


@pytest.fixture(scope="module")
def runs(folders):
    done = {}

    def get(mode):
        if mode not in done:
            done[mode] = run(folders, mode, mode)
        return done[mode]
    return get


def test_fit_and_test_equal_features_mode(runs):
    fr, fe = runs("frames"), runs("features")
    assert fr["mod"].net.load_from_features is False and fe["mod"].net.load_from_features is True
    assert fr["weights"].keys() == fe["weights"].keys()
    for n, w in fe["weights"].items():
        assert torch.equal(fr["weights"][n], w), n
    trained = [n for n, p in fr["mod"].net.named_parameters() if p.requires_grad]
    fresh = dict(build_net(False).named_parameters())
    assert trained and any(not torch.equal(fr["weights"][n], fresh[n]) for n in trained)       # (the run did train)
    for rel in ("save/ncentroid.pt", "logs/train/runs/checkpoints/ncentroid.pt"):
        assert torch.equal(torch.load(fr["base"] / rel), torch.load(fe["base"] / rel)), rel
    for rel in ("save/metrics_0.json", "save/metrics_1.json", "logs/eval/runs/checkpoints/metrics.json"):
        a, b = (fr["base"] / rel).read_text(), (fe["base"] / rel).read_text()
        assert a == b and "auc_roc" in json.loads(a), rel
    assert fr["metrics"] and json.dumps(fr["metrics"], sort_keys=True) == json.dumps(fe["metrics"], sort_keys=True)
    dm = fr["dm"]
    assert len(dm.bank) == 6 and len(dm._test_bank) == 2 and dm._normal_bank is None and not list((fr["base"]).rglob("*.npy"))


def test_score_videos_group_of_tiles(runs):
    """a group of three tiles goes through ONE acx_tile_videos launch into forward_test_many; against three _score_video calls and
    against the same group handed over as tensors"""
    r = runs("frames")
    mod, dm = r["mod"], r["dm"]
    mod.net.eval()
    batches = list(dm.train_dataloader_test_mode())
    assert len(batches) == 3 and all(isinstance(b[0], BankTile) and b[0].bank is dm.bank for b in batches)
    calls = []
    real = ops.tile_videos

    def counting(*a, **k):
        calls.append(list(a[3]))
        return real(*a, **k)
    ops.tile_videos = counting
    try:
        group = mod.score_videos(batches)
    finally:
        ops.tile_videos = real
    assert calls == [[0, 1, 2]]
    tensors = mod.score_videos([(b[0].to(DEV),) + tuple(b[1:]) for b in batches])
    single = [mod._score_video(b) for b in batches]
    for k, (g, t, s, (_, n, a, b, _)) in enumerate(zip(group, tensors, single, NORMAL)):
        assert g[0].shape == (b - a + 1,) and g[2].shape == (b - a + 1, NUM_CLASSES - 1)
        for x, y, z in zip(g, t, s):
            print(f"video {k}: max |group - single| = {(x.double() - z.double()).abs().max().item():.3g}")
            assert torch.equal(x, y)
            assert torch.equal(x, z)


def test_resume_in_frames_mode(folders, runs):
    """last.ckpt of a one-epoch frames-mode run, resumed in a fresh module and datamodule under other seeds for the second epoch:
    the weights of the uninterrupted two-epoch run"""
    want = runs("frames")["weights"]
    first = run(folders, "frames", "resume_first", max_epochs=1, test=False)
    ck = torch.load(first["ckpt"], map_location="cpu", weights_only=False)
    assert ck["epoch"] == 0 and ck["global_step"] == 3
    second = run(folders, "frames", "resume_second", max_epochs=2, ckpt_path=first["ckpt"], test=False, seeds=(5, 6))
    for n, w in want.items():
        assert torch.equal(second["weights"][n], w), n
