"""-m gpu: training batches from a feature set resident in device memory.  The gather kernel against the formula in numpy
(acx_sample_segments is a pure copy: every comparison here is bit for bit), the resident loader against batches the REFERENCE's
train-mode dataset produced (tests/golden/train_batches.npz), a bank past 2^31 floats, the ncentroid fast path against the loader
path, and Trainer.fit fed by the datamodule against the same fit fed by host-built batches."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib, ops
from anomalyclip_amd import feature_index as FI
from anomalyclip_amd.datamodule import AnomalyCLIPDataModule
from anomalyclip_amd.feature_bank import FeatureBank, ResidentTrainLoader
from anomalyclip_amd.trainer import Trainer
import recipes_train as RT

DEV = torch.device("cuda", 0)


def gather_reference(files, ncrops, vid, starts, N, L, stride):
    """the formula of include/acx.h in numpy: files[v] is [T_v * ncrops, D] as stored -> [B, ncrops, N * L, D]"""
    out = []
    for b, v in enumerate(vid):
        f = files[v].reshape(-1, ncrops, files[v].shape[-1])
        idx = FI.frame_index_table(np.asarray(starts[b * N:(b + 1) * N], dtype=np.int64), L, stride, f.shape[0])
        out.append(f[idx].transpose(1, 0, 2))
    return np.stack(out)


def device_tables(files):
    rows = [f.shape[0] for f in files]
    off = np.concatenate([[0], np.cumsum(rows)[:-1]]).astype(np.int64)
    return torch.from_numpy(np.concatenate(files)).to(DEV), torch.from_numpy(off).to(DEV)


def i32(a):
    return torch.tensor(np.asarray(a, dtype=np.int32)).to(DEV)


# ====================================================================================================== the kernel
@pytest.mark.parametrize("D", [4, 512, 640, 768, 1024])
@pytest.mark.parametrize("ncrops,stride", [(1, 1), (2, 3)])
def test_sample_segments_matches_formula(D, ncrops, stride):
    """videos of 1, 5, 37 and 300 frames; a batch with the same video twice; starts up to several times past T (T = 1, T = 5 with
    L = 16); 9 * ncrops * 80 output rows: more than one workgroup, a row count that is no multiple of a workgroup's 16 rows"""
    rng = np.random.default_rng(D + ncrops)
    T = [1, 5, 37, 300]
    files = [rng.standard_normal((t * ncrops, D)).astype(np.float32) for t in T]
    N, L = 5, 16
    vid = [2, 0, 3, 1, 2, 2, 0, 3, 1]
    starts = rng.integers(0, 400, size=len(vid) * N)
    bank, row_off = device_tables(files)
    out = ops.sample_segments(bank, row_off, i32(T), i32(vid), i32(starts), N, L, stride, ncrops)
    assert out.shape == (len(vid), ncrops, N * L, D) and out.dtype == torch.float32
    assert np.array_equal(out.cpu().numpy(), gather_reference(files, ncrops, vid, starts, N, L, stride))
    # into a caller's buffer; one video, one segment, one frame
    buf = torch.full((1, ncrops, 1, D), -1.0, device=DEV)
    assert ops.sample_segments(bank, row_off, i32(T), i32([3]), i32([299]), 1, 1, stride, ncrops, out=buf) is buf
    assert np.array_equal(buf.cpu().numpy(), gather_reference(files, ncrops, [3], [299], 1, 1, stride))


def test_sample_segments_grid_stride():
    """more rows than one sweep of the capped grid covers (2048 workgroups x 16 rows): 40,000 rows of 4 floats"""
    files = [np.arange(7 * 4, dtype=np.float32).reshape(7, 4), np.arange(3 * 4, dtype=np.float32).reshape(3, 4) + 100]
    N, L, B = 50, 8, 100
    vid = np.arange(B) % 2
    starts = np.arange(B * N) * 3
    bank, row_off = device_tables(files)
    out = ops.sample_segments(bank, row_off, i32([7, 3]), i32(vid), i32(starts), N, L, 2, 1)
    assert np.array_equal(out.cpu().numpy(), gather_reference(files, 1, vid, starts, N, L, 2))


def test_sample_segments_empty_batch_and_bad_width():
    files = [np.ones((4, 8), dtype=np.float32)]
    bank, row_off = device_tables(files)
    out = ops.sample_segments(bank, row_off, i32([4]), i32([]), i32([]), 3, 2, 1, 1)
    assert out.shape == (0, 1, 6, 8)
    bank6 = torch.ones(4, 6, device=DEV)
    with pytest.raises(_lib.AcxError, match="acx_sample_segments"):
        ops.sample_segments(bank6, row_off, i32([4]), i32([0]), i32([0, 1, 2]), 3, 2, 1, 1)
    torch.cuda.synchronize()


def test_sample_segments_past_2_31_floats():
    """a bank of 2^31 + 40 * 512 floats (8.6 GB, never filled): its last 40 rows are one video; offsets must be 64-bit"""
    D, T = 512, 40
    rows = (1 << 31) // D + T
    bank = torch.empty(rows, D, dtype=torch.float32, device=DEV)
    assert bank.numel() > 1 << 31
    video = np.random.default_rng(0).standard_normal((T, D)).astype(np.float32)
    bank[rows - T:].copy_(torch.from_numpy(video))
    N, L = 4, 16
    starts = [0, 30, 39, 77]
    out = ops.sample_segments(bank, torch.tensor([rows - T], dtype=torch.int64, device=DEV), i32([T]), i32([0, 0]), i32(starts * 2),
                              N, L, 1, 1)
    assert np.array_equal(out.cpu().numpy(), gather_reference([video], 1, [0, 0], starts * 2, N, L, 1))
    del bank, out
    torch.cuda.empty_cache()


# ====================================================================================================== bank + loader
@pytest.mark.parametrize("name", sorted(RT.CASES))
def test_resident_loader_equals_reference_batches(name, tmp_path, golden):
    """both epochs of the reference's DataLoader(shuffle=True, drop_last=True, batch_size=2) over its train-mode dataset"""
    case, g = RT.CASES[name], golden("train_batches")
    ann, paths, frames, labels = RT.write_case(tmp_path, case)
    bank = FeatureBank(paths, frames, labels, case["ncrops"], DEV)
    assert bank.bank.shape == (sum(case["T"]) * case["ncrops"], RT.D) and bank.frames.tolist() == list(case["T"])
    assert bank.labels.tolist() == labels and bank.row_off.dtype == torch.int64 and bank.paths == paths
    for v, p in enumerate(paths):
        assert np.array_equal(bank.video(v).cpu().numpy(), np.load(p))
    torch.manual_seed(RT.TORCH_SEED)
    np.random.seed(RT.NUMPY_SEED)
    loader = ResidentTrainLoader(bank, range(len(paths)), RT.BATCH, case["N"], case["L"], case["stride"])
    k = 0
    for _ in range(RT.EPOCHS):
        for feats, lab in loader:
            assert feats.device == DEV and lab.device == DEV and lab.dtype == torch.int64 and feats.is_contiguous()
            assert np.array_equal(feats.cpu().numpy(), g[f"{name}_feat{k}"]), (name, k)
            assert np.array_equal(lab.cpu().numpy(), g[f"{name}_label{k}"]), (name, k)
            k += 1
    assert k == int(g[f"{name}_batches"]) == RT.EPOCHS * len(loader)


def test_feature_bank_refuses_what_it_cannot_hold(tmp_path):
    ann, paths, frames, labels = RT.write_case(tmp_path, RT.CASES["A"])
    with pytest.raises(ValueError, match=r"need \d+ bytes.*1024 bytes"):
        FeatureBank(paths, frames, labels, 1, DEV, max_bytes=1024)
    np.save(tmp_path / "f64.npy", np.zeros((3, 8)))
    with pytest.raises(ValueError, match="f64.npy"):
        FeatureBank([str(tmp_path / "f64.npy")], [3], [0], 1, DEV)
    np.save(tmp_path / "d3.npy", np.zeros((2, 3, 8), dtype=np.float32))
    with pytest.raises(ValueError, match="d3.npy"):
        FeatureBank([str(tmp_path / "d3.npy")], [2], [0], 1, DEV)


def test_feature_bank_load_in_several_staging_groups(tmp_path, monkeypatch):
    """files that do not fit one staging slot together: several groups, both slots reused"""
    from anomalyclip_amd import feature_bank as FB
    monkeypatch.setattr(FB, "_STAGE_BYTES", 4096)
    rng = np.random.default_rng(1)
    arrays = [rng.standard_normal((t, 16)).astype(np.float32) for t in (40, 3, 70, 64, 1, 9, 33)]
    paths = []
    for i, a in enumerate(arrays):
        paths.append(str(tmp_path / f"g{i}.npy"))
        np.save(paths[-1], a)
    bank = FeatureBank(paths, [len(a) for a in arrays], [0] * len(arrays), 1, DEV, readers=3)
    assert np.array_equal(bank.bank.cpu().numpy(), np.concatenate(arrays))


# ====================================================================================================== datamodule, module, trainer
NORMAL_ID = 7


def write_dataset(root, normal_T, anomaly_T, anomaly_labels, D=512):
    """feature files ~ N(0.1, 0.3^2) and the reference's list files -> datamodule hyper-parameters"""
    rng = np.random.default_rng(42)
    lists = {}
    for kind, Ts, labs in (("normal", normal_T, [NORMAL_ID] * len(normal_T)), ("anomaly", anomaly_T, anomaly_labels)):
        lists[kind] = str(root / f"{kind}.txt")
        with open(lists[kind], "w") as fh:
            for i, (T, lab) in enumerate(zip(Ts, labs)):
                np.save(root / f"{kind}{i}_{T}.npy", (rng.standard_normal((T, D)) * 0.3 + 0.1).astype(np.float32))
                fh.write(f"{kind}{i}_{T} 0 {T - 1} {lab}\n")
    return dict(frames_root=str(root), annotation_file_normal=lists["normal"], annotation_file_anomaly=lists["anomaly"],
                annotation_file_test=lists["anomaly"], annotation_file_temporal_test=None, labels_file=None, normal_id=NORMAL_ID,
                num_classes=14, device=DEV)


@pytest.fixture(scope="module")
def grid_modules():
    """two modules of the 24 x 10 head (the smallest grid test_gpu_head_grid.py trains) from the same seed"""
    from test_gpu_head_grid import FULL, _grid_module
    hc = FULL["24x10"]
    return hc, [_grid_module(hc) for _ in range(2)]


def test_ncentroid_fast_path_bit_identical_to_loader_path(tmp_path, grid_modules):
    hc, mods = grid_modules
    mod = mods[0][0]
    hp = write_dataset(tmp_path, (5, 513, 1025), (30,), (3,))
    dm = AnomalyCLIPDataModule(**hp, num_segments=hc.num_segments, seg_length=hc.seg_length, batch_size=2)
    dm.setup("fit")
    slow = mod.compute_ncentroid(dm.train_dataloader_test_mode()).clone()
    videos = dm.resident_normal_videos()
    assert [v.shape[0] for v in videos] == [5, 513, 1025]
    fast = mod.compute_ncentroid_resident(videos).clone()
    assert torch.equal(fast, slow)
    want = np.concatenate([np.load(r.path) for r in dm.normal]).astype(np.float64).mean(0)
    assert np.abs(fast.cpu().numpy() - want).max() < 1e-6
    # several crops or a stride: the bank's rows are not the loader's rows, the module takes the loader path
    dm.hparams.stride = 2
    assert dm.resident_normal_videos() is None


def test_fit_from_datamodule_bit_identical_to_host_batches(tmp_path, grid_modules):
    """Trainer(max_epochs=1, limit_train_batches=2).fit over eight feature files: the losses of both steps and every parameter
    afterwards equal those of the same fit fed by a plain list of batches built on the host (feature_index) and moved with .to()"""
    hc, mods = grid_modules
    N, L, B = hc.num_segments, hc.seg_length, 4
    hp = write_dataset(tmp_path, (5, 241, 300, 700), (240, 1, 999, 64), (1, 13, 3, 5))
    hp.update(num_segments=N, seg_length=L, batch_size=B)
    g = torch.Generator().manual_seed(9)
    masks = [torch.bernoulli(torch.ones(B, N) * 0.3, generator=g) for _ in range(2)]
    for m in masks:
        m[:, :hc.num_topk] = 1

    def fit(mod, net, dm, save_dir):
        mod.hparams["save_dir"] = str(save_dir)
        net.selector_model.generate_mask = lambda b: (masks[0], masks[1])
        losses, step = [], mod.train_batch

        def recording(batch, opt, i=0):
            r = step(batch, opt, i)
            losses.append(torch.stack([torch.as_tensor(v).detach().reshape(()) for v in mod.last_losses]).clone())
            return r
        mod.train_batch = recording
        try:
            Trainer(max_epochs=1, limit_train_batches=2, check_val_every_n_epoch=2).fit(mod, dm)
        finally:
            del mod.train_batch
        torch.cuda.synchronize()
        return losses, {n: p.detach().clone() for n, p in net.named_parameters()}

    # (a) the host plan: the same samplers and draws, rows gathered with numpy
    dm_host = AnomalyCLIPDataModule(**hp)
    dm_host.setup("test")                                        # lists only, no bank
    recs = dm_host.normal + dm_host.anomaly
    host_bank = SimpleNamespace(paths=[r.path for r in recs], num_frames=[r.num_frames for r in recs], ncrops=1,
                                labels_host=np.asarray([r.label for r in recs], dtype=np.int64), file_frames=None)
    files = [np.load(r.path) for r in recs]
    torch.manual_seed(77)
    np.random.seed(78)
    plans = [ResidentTrainLoader(host_bank, ids, B // 2, N, L, 1).host_batches() for ids in (range(4), range(4, 8))]
    host = [[], []]
    for _ in range(2):                                           # the trainer's order: normal batch, abnormal batch, per step
        for k in range(2):
            vid, starts, labels = next(plans[k])
            feats = torch.from_numpy(gather_reference(files, 1, vid, starts, N, L, 1)).pin_memory()
            host[k].append((feats, torch.from_numpy(labels)))
    dm_list = SimpleNamespace(hparams=dm_host.hparams, num_classes=14, setup=lambda stage: None, train_dataloader=lambda: host,
                              train_dataloader_test_mode=dm_host.train_dataloader_test_mode)
    want_losses, want_params = fit(*mods[1], dm_list, tmp_path / "host")

    # (b) the datamodule: bank + gather kernel, under the same seeds
    torch.manual_seed(77)
    np.random.seed(78)
    dm = AnomalyCLIPDataModule(**hp)
    got_losses, got_params = fit(*mods[0], dm, tmp_path / "resident")
    assert dm.bank is not None and len(dm.bank) == 8 and len(got_losses) == len(want_losses) == 2
    for a, b in zip(got_losses, want_losses):
        assert torch.isfinite(a).all() and torch.equal(a, b), (a, b)
    for n in want_params:
        assert torch.equal(got_params[n], want_params[n]), n
    assert torch.equal(mods[0][0].ncentroid, mods[1][0].ncentroid)
