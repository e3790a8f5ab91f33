"""-m gpu: half-precision feature files.  The cast against numpy.astype(float16) bit for bit, the two gathers on a float16 bank
against the same gathers on the float32 bank of the same values (a half widens exactly: every comparison is torch.equal), the
stream, the extractor, and whole fit / test runs on float16 files against the same runs on their widened float32 copies.

The designated fail-before test is test_bank_from_float16_files: on the parent commit FeatureBank refuses a '<f2' file with
"feature files must be C-ordered float32".  Every other test here that passes a float16 file, dtype= or bank_dtype= fails there
too (ValueError, TypeError, or a missing symbol)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import feature_f16_ref as F
from anomalyclip_amd import _lib, ops
from anomalyclip_amd import extract as X
from anomalyclip_amd import feature_index as FI
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd.datamodule import AnomalyCLIPDataModule
from anomalyclip_amd.feature_bank import BankTile, FeatureBank, ResidentTrainLoader
from anomalyclip_amd.feature_stream import FeatureStream
from anomalyclip_amd.trainer import Trainer
import recipes as R
from test_gpu_extract import _tiny_vit, _video
from test_gpu_feature_bank import i32
from test_gpu_frames_mode import build_module, folders  # noqa: F401  (the frame folders and list files of the frames-mode tests)

DEV = torch.device("cuda", 0)


# ====================================================================================================== the cast
@pytest.fixture(scope="module")
def cast_data():
    x = F.cast_inputs()
    return x, torch.from_numpy(x).to(DEV)


def _cast(src):
    over = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = ops.cast_rows_f16(src, over)
    return out.cpu().numpy(), int(over.item())


def test_cast_bit_for_bit_numpy_one_launch(cast_data):
    """the crafted vector and 14 x 4096 scaled normals in ONE launch (260 columns: a second lane stride with one live lane)"""
    x, xd = cast_data
    n = x.size // 260 * 260
    assert n >= F.crafted_floats().size + 13 * 4096                    # (the tail cut off is part of the last decade only)
    got, over = _cast(xd[:n].view(-1, 260))
    want = F.to_half(x[:n]).reshape(-1, 260)
    bad = np.flatnonzero(got.view(np.int16).ravel() != want.view(np.int16).ravel())
    assert bad.size == 0, [(float(x[i]), hex(int(x[i:i + 1].view(np.uint32)[0])), hex(int(got.view(np.uint16).ravel()[i])),
                            hex(int(want.view(np.uint16).ravel()[i]))) for i in bad[:8]]
    assert over == F.overflow_count(x[:n]) and over > 100             # the 1e5 decade alone overflows often
    # the rest of the vector, as 4-wide rows
    tail = x[n:n + (x.size - n) // 4 * 4]
    got, over = _cast(xd[n:n + tail.size].view(-1, 4))
    assert np.array_equal(got.view(np.int16), F.to_half(tail).reshape(-1, 4).view(np.int16)) and over == F.overflow_count(tail)


@pytest.mark.parametrize("cols", [4, 8, 12, 260])
@pytest.mark.parametrize("rows", [1, 3, 5])
def test_cast_shapes_and_row_stride(cast_data, rows, cols):
    """rows 1, 3, 5: the tail of a four-rows-per-wave unit; ld > cols: the rows of a wider matrix.  The crafted values lead the
    vector, so the small shapes hold them"""
    x, xd = cast_data
    ld = cols + 8
    src = xd[:rows * ld].view(rows, ld)[:, :cols]
    assert src.stride(0) == ld and src.shape == (rows, cols)
    got, over = _cast(src)
    ref = x[:rows * ld].reshape(rows, ld)[:, :cols]
    assert got.shape == (rows, cols) and np.array_equal(got.view(np.int16), F.to_half(ref).view(np.int16))
    assert over == F.overflow_count(ref)
    # into a caller's buffer, adding to a counter that already holds something
    buf = torch.zeros(rows + 1, cols, dtype=torch.float16, device=DEV)
    cnt = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    assert ops.cast_rows_f16(src, cnt, out=buf[:rows]).data_ptr() == buf.data_ptr()
    assert np.array_equal(buf[:rows].cpu().numpy().view(np.int16), F.to_half(ref).view(np.int16)) and int(cnt) == 7 + over
    assert not buf[rows].any()                                         # nothing past the last row


def test_cast_no_rows_is_a_no_op():
    over = torch.full((1,), 3, dtype=torch.int64, device=DEV)
    out = ops.cast_rows_f16(torch.empty(0, 8, device=DEV), over)
    assert out.shape == (0, 8) and out.dtype == torch.float16 and int(over) == 3


def test_expand_rows_is_exact():
    h = F.random_halves((37, 260), 5)
    d = torch.from_numpy(h).to(DEV)
    out = ops.expand_rows_f16(d)
    assert out.dtype == torch.float32 and np.array_equal(out.cpu().numpy(), h.astype(np.float32))
    assert ops.expand_rows_f16(d[:0]).shape == (0, 260)
    with pytest.raises(_lib.AcxError, match="acx_expand_rows_f16"):
        ops.expand_rows_f16(torch.zeros(3, 6, dtype=torch.float16, device=DEV))
    torch.cuda.synchronize()


# ====================================================================================================== the gathers
def _banks(T, ncrops, D, seed):
    """float16 bank of random finite halves, the float32 bank of the same values, row offsets"""
    rows = [t * ncrops for t in T]
    h = F.random_halves((sum(rows), D), seed)
    off = np.concatenate([[0], np.cumsum(rows)[:-1]]).astype(np.int64)
    return torch.from_numpy(h).to(DEV), torch.from_numpy(h.astype(np.float32)).to(DEV), torch.from_numpy(off).to(DEV)


@pytest.mark.parametrize("D", [4, 12, 260, 512])
@pytest.mark.parametrize("ncrops,stride", [(1, 1), (2, 2), (1, 2), (2, 1)])
def test_gathers_on_a_half_bank_equal_the_float_bank(D, ncrops, stride):
    """D = 12: rows at 8 mod 16 bytes; D = 260: D / 4 = 65, a second lane stride with one live lane.  45 * ncrops output rows: three
    workgroups and no multiple of four; a negative start and starts past T (the true modulus); T = 1"""
    T = [1, 5, 37, 300]
    b16, b32, row_off = _banks(T, ncrops, D, D + ncrops)
    frames = i32(T)
    N, L = 3, 5
    vid = [2, 0, 3]
    starts = [-7, 0, 36, 4, 9, 1, 299, 1000, -301]
    got = ops.sample_segments(b16, row_off, frames, i32(vid), i32(starts), N, L, stride, ncrops)
    want = ops.sample_segments(b32, row_off, frames, i32(vid), i32(starts), N, L, stride, ncrops)
    assert got.dtype == torch.float32 and got.shape == (3, ncrops, N * L, D) and torch.equal(got, want)
    # the rows are the rows of the formula, not only those of the float32 kernel
    f = b32[int(row_off[3]):].view(300, ncrops, D)
    t = [(299 + l * stride) % 300 for l in range(L)]
    assert torch.equal(got[2, :, :L], f[t].transpose(0, 1))
    t = [(-301 + l * stride) % 300 for l in range(L)]
    assert torch.equal(got[2, :, 2 * L:], f[t].transpose(0, 1))
    buf = torch.full_like(got, -1.0)
    assert ops.sample_segments(b16, row_off, frames, i32(vid), i32(starts), N, L, stride, ncrops, out=buf) is buf and torch.equal(buf, want)
    assert ops.sample_segments(b16, row_off, frames, i32([]), i32([]), N, L, stride, ncrops).shape == (0, ncrops, N * L, D)
    # the test-mode tiles of the four videos in one launch, one of them twice
    vids = [3, 0, 1, 2, 3]
    S = [FI.test_start_indices(T[v], 2, 3, stride)[1] for v in vids]
    got = ops.tile_videos(b16, row_off, frames, vids, S, 2, 3, stride, ncrops)
    want = ops.tile_videos(b32, row_off, frames, vids, S, 2, 3, stride, ncrops)
    assert got.dtype == torch.float32 and got.shape == (ncrops * 6 * sum(S), D) and torch.equal(got, want)
    buf = torch.full_like(got, -1.0)
    assert ops.tile_videos(b16, row_off, frames, vids, S, 2, 3, stride, ncrops, out=buf) is buf and torch.equal(buf, want)
    assert ops.tile_videos(b16, row_off, frames, [], [], 2, 3, stride, ncrops).shape == (0, D)


def test_gathers_grid_stride_on_a_half_bank():
    """more rows than one sweep of the capped grid covers (2048 workgroups x 16 rows): 40,000 rows of 4 halves"""
    b16, b32, row_off = _banks([7, 3], 1, 4, 1)
    N, L, B = 50, 8, 100
    vid, starts = i32(np.arange(B) % 2), i32(np.arange(B * N) * 3)
    a = ops.sample_segments(b16, row_off, i32([7, 3]), vid, starts, N, L, 2, 1)
    assert torch.equal(a, ops.sample_segments(b32, row_off, i32([7, 3]), vid, starts, N, L, 2, 1))


def test_half_bank_slices_8_byte_aligned_accepted_4_byte_refused():
    """a bank slice that starts an odd number of 12-wide rows in is 8-byte, not 16-byte aligned: accepted and exact; a base that is
    only 4-byte aligned is refused by name"""
    T = [5, 9]
    b16, b32, row_off = _banks(T, 1, 12, 3)
    extra16 = torch.cat([b16[:1], b16])[1:]                             # the same rows, one row into another allocation
    assert extra16.data_ptr() % 16 == 8 and extra16.is_contiguous()
    frames, vid, starts = i32(T), i32([1, 0]), i32([3, 8, 0, 4])
    want = ops.sample_segments(b32, row_off, frames, vid, starts, 2, 3, 1, 1)
    assert torch.equal(ops.sample_segments(extra16, row_off, frames, vid, starts, 2, 3, 1, 1), want)
    S = [FI.test_start_indices(t, 2, 3, 1)[1] for t in T]
    assert torch.equal(ops.tile_videos(extra16, row_off, frames, [0, 1], S, 2, 3, 1, 1),
                       ops.tile_videos(b32, row_off, frames, [0, 1], S, 2, 3, 1, 1))
    flat = torch.zeros(14 * 12 + 8, dtype=torch.float16, device=DEV)
    odd = flat[2:2 + 14 * 12].view(14, 12)
    assert odd.data_ptr() % 8 == 4 and odd.is_contiguous()
    with pytest.raises(_lib.AcxError, match="acx_sample_segments_f16"):
        ops.sample_segments(odd, row_off, frames, vid, starts, 2, 3, 1, 1)
    with pytest.raises(_lib.AcxError, match="acx_tile_videos_f16"):
        ops.tile_videos(odd, row_off, frames, [0, 1], S, 2, 3, 1, 1)
    with pytest.raises(_lib.AcxError, match="acx_sample_segments_f16"):
        ops.sample_segments(torch.zeros(14, 6, dtype=torch.float16, device=DEV), row_off, frames, vid, starts, 2, 3, 1, 1)
    with pytest.raises(TypeError, match="float32 or float16"):
        ops.sample_segments(b32.to(torch.bfloat16), row_off, frames, vid, starts, 2, 3, 1, 1)
    with pytest.raises(TypeError, match="float32 or float16"):
        ops.tile_videos(b32.double(), row_off, frames, [0, 1], S, 2, 3, 1, 1)
    torch.cuda.synchronize()


def test_half_bank_past_2_31_elements():
    """a bank of 2^31 + 40 * 512 halves (4.3 GB, never filled): its last 40 rows are one video that lies past the boundary as a
    whole; both gathers against the float32 gathers on those 40 rows alone.  Element offsets must be 64-bit."""
    D, T = 512, 40
    rows = (1 << 31) // D + T
    bank = torch.empty(rows, D, dtype=torch.float16, device=DEV)
    assert bank.numel() > 1 << 31 and (rows - T) * D >= 1 << 31
    h = F.random_halves((T, D), 0)
    bank[rows - T:].copy_(torch.from_numpy(h))
    small = torch.from_numpy(h.astype(np.float32)).to(DEV)
    zero = torch.zeros(1, dtype=torch.int64, device=DEV)
    N, L = 4, 16
    starts = [0, 30, 39, 77]
    off = torch.tensor([rows - T], dtype=torch.int64, device=DEV)
    got = ops.sample_segments(bank, off, i32([T]), i32([0, 0]), i32(starts * 2), N, L, 1, 1)
    assert torch.equal(got, ops.sample_segments(small, zero, i32([T]), i32([0, 0]), i32(starts * 2), N, L, 1, 1))
    off2 = torch.tensor([0, rows - T], dtype=torch.int64, device=DEV)
    S = FI.test_start_indices(T, 4, 4, 1)[1]
    got = ops.tile_videos(bank, off2, i32([7, T]), [1, 1], [S, S], 4, 4, 1, 1)
    assert torch.equal(got, ops.tile_videos(small, zero, i32([T]), [0, 0], [S, S], 4, 4, 1, 1))
    del bank, got
    torch.cuda.empty_cache()


# ====================================================================================================== bank and loaders from files
def _write_pair(root, Ts, ncrops, D, seed):
    """float16 files of seeded normals and the float32 files of the same (rounded) values -> (paths16, paths32, the arrays)"""
    p16, p32, arrays = [], [], []
    for i, T in enumerate(Ts):
        h = np.random.default_rng(seed + i).standard_normal((T * ncrops, D)).astype(np.float16)
        arrays.append(h)
        p16.append(str(root / f"h{i}_{T}.npy"))
        p32.append(str(root / f"f{i}_{T}.npy"))
        np.save(p16[-1], h)
        np.save(p32[-1], h.astype(np.float32))
    return p16, p32, arrays


def test_bank_from_float16_files(tmp_path, monkeypatch):
    """THE fail-before test: a bank over '<f2' files holds halves (dtype, nbytes, the max_bytes check and the staging slots by the
    real element size), video() is a view in that dtype, and the train loader and the test tiles are float32, equal to those of the
    float32 files' bank"""
    from anomalyclip_amd import feature_bank as FB
    monkeypatch.setattr(FB, "_STAGE_BYTES", 4096)                      # several staging groups, both slots reused
    Ts = (40, 3, 70, 64, 1, 9, 33)
    p16, p32, arrays = _write_pair(tmp_path, Ts, 2, 16, 11)
    frames, labels = list(Ts), [7, 7, 7, 1, 2, 3, 4]
    need = sum(Ts) * 2 * 16 * 2
    with pytest.raises(ValueError, match=rf"need {need} bytes.*{need - 1} bytes"):
        FeatureBank(p16, frames, labels, 2, DEV, max_bytes=need - 1)
    b16 = FeatureBank(p16, frames, labels, 2, DEV, max_bytes=need, readers=3)
    b32 = FeatureBank(p32, frames, labels, 2, DEV)
    assert b16.dtype == torch.float16 and b16.bank.dtype == torch.float16 and b16.nbytes == need and b32.nbytes == 2 * need
    assert b32.dtype == torch.float32 and b16.bank.shape == b32.bank.shape
    assert np.array_equal(b16.bank.cpu().numpy().view(np.int16), np.concatenate(arrays).view(np.int16))
    for v, a in enumerate(arrays):
        assert b16.video(v).dtype == torch.float16 and np.array_equal(b16.video(v).cpu().numpy(), a)
    with pytest.raises(ValueError, match=r"f2_70\.npy"):
        FeatureBank(p16[:2] + p32[2:], frames, labels, 2, DEV)
    out = []
    for bank in (b16, b32):
        torch.manual_seed(3)
        loader = ResidentTrainLoader(bank, [0, 2, 3, 6], 2, 4, 3, 2, rng=np.random.RandomState(4))
        out.append([(f.clone(), l.clone()) for f, l in loader])
    assert len(out[0]) == len(out[1]) == 2
    for (fa, la), (fb, lb) in zip(*out):
        assert fa.dtype == torch.float32 and fa.shape == (2, 2, 12, 16) and torch.equal(fa, fb) and torch.equal(la, lb)
    for v in range(len(Ts)):
        ta, tb = BankTile(b16, v, 4, 3, 2), BankTile(b32, v, 4, 3, 2)
        assert ta.shape == tb.shape and ta.to(DEV).dtype == torch.float32 and torch.equal(ta.to(DEV), tb.to(DEV))


@pytest.mark.parametrize("ncrops,stride", [(1, 1), (2, 1), (1, 2)])
def test_stream_of_float16_files_equals_float32_files(tmp_path, ncrops, stride):
    """37 frames: shorter than one 512-frame tile (the rows wrap around); 513 and 1030: two and three tiles"""
    Ts = (37, 513, 1030, 5)
    p16, p32, arrays = _write_pair(tmp_path, Ts, ncrops, 32, 21)
    kw = dict(ncrops=ncrops, stride=stride, device=DEV)
    one16, one32 = list(FeatureStream(p16, **kw)), list(FeatureStream(p32, **kw))
    assert len(one16) == len(one32) == 4
    for (a, Ta, Sa, pa), (b, Tb, Sb, pb), T, arr in zip(one16, one32, Ts, arrays):
        assert a.dtype == torch.float32 and a.shape == b.shape == (1, ncrops, 512 * Sa, 32) and (Ta, Sa) == (Tb, Sb) == (T, Sa)
        assert torch.equal(a, b)
        want, S = FI.gather_test_features(arr.astype(np.float32), 32, 16, stride, ncrops)
        assert S == Sa and np.array_equal(a.cpu().numpy()[0], want)
    g16, g32 = list(FeatureStream(p16, **kw).batched(videos=3)), list(FeatureStream(p32, **kw).batched(videos=3))
    assert len(g16) == len(g32) >= 2
    for (a, ma), (b, mb) in zip(g16, g32):
        assert a.dtype == torch.float32 and torch.equal(a, b)
        assert [m[:3] for m in ma] == [m[:3] for m in mb]
    # a group that mixes the two kinds of file is widened on the host, file by file
    mixed = list(FeatureStream([p16[0], p32[1], p16[2], p32[3]], **kw).batched(videos=4, first=4))
    flat = torch.cat([x for x, _ in mixed])
    assert torch.equal(flat, torch.cat([x for x, _ in g32]))


# ====================================================================================================== the extractor
@pytest.fixture(scope="module")
def clip_frames(tmp_path_factory):
    root = tmp_path_factory.mktemp("f16_frames")
    lens = {"a/v40": 40, "a/v300": 300, "b/v7": 7}
    for i, (v, T) in enumerate(lens.items()):
        _video(os.path.join(str(root), v), T, (48, 64), "jpg", seed=50 + i)
    return str(root), lens


@pytest.mark.parametrize("pack", [False, True])
@pytest.mark.parametrize("ncrops", [1, 5])
def test_extract_float16_files_are_the_rounded_float32_files(tmp_path, clip_frames, ncrops, pack):
    """the same launches either way, so the float16 file's bytes are numpy's rounding of the float32 file's"""
    root, lens = clip_frames
    enc, _ = _tiny_vit()
    o32, o16 = str(tmp_path / "f32"), str(tmp_path / "f16")
    want = {"written": 3, "skipped": 0, "frames": sum(lens.values()), "rows": sum(lens.values()) * ncrops}
    assert X.extract_dataset(enc, None, root, o32, ncrops=ncrops, pack=pack) == want
    assert X.extract_dataset(enc, None, root, o16, ncrops=ncrops, pack=pack, dtype="float16") == want
    for v, T in lens.items():
        a, b = np.load(os.path.join(o32, v + ".npy")), np.load(os.path.join(o16, v + ".npy"))
        assert b.dtype == np.float16 and b.shape == a.shape == (T * ncrops, 128) and b.flags.c_contiguous
        assert np.array_equal(b.view(np.int16), a.astype(np.float16).view(np.int16))
        assert os.path.getsize(os.path.join(o16, v + ".npy")) == 128 + b.size * 2 and not os.path.exists(os.path.join(o16, v + ".npy.tmp"))
    # complete float16 files are kept; asked for as float32 they are rewritten, never kept silently
    again = X.extract_dataset(enc, None, root, o16, ncrops=ncrops, pack=pack, dtype="float16")
    assert again["written"] == 0 and again["skipped"] == 3
    assert X.extract_dataset(enc, None, root, o16, ncrops=ncrops, pack=pack)["written"] == 3
    assert np.array_equal(np.load(os.path.join(o16, "b/v7.npy")), np.load(os.path.join(o32, "b/v7.npy")))
    if not pack and ncrops == 1:
        r = X.extract_video(enc, X.FrameFolderReader(root, "b/v7"), str(tmp_path / "one"), dtype="float16")
        assert r == {"written": True, "frames": 7, "rows": 7}
        assert np.array_equal(np.load(str(tmp_path / "one.npy")), np.load(os.path.join(o32, "b/v7.npy")).astype(np.float16))


@pytest.mark.parametrize("pack", [False, True])
def test_extract_refuses_features_no_half_holds(tmp_path, clip_frames, pack):
    """an output projection scaled until features pass 65504: ValueError naming the video and the count, nothing under the final
    name (a ValueError raised on the host from a counter, not a device fault)"""
    root, lens = clip_frames
    enc = X.build_image_encoder("tiny", "f32")
    sd = IW.init_vit_state_dict(IW.TINY, 13, prefix="")
    sd["proj"] = sd["proj"] * 3.0e5
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(DEV).eval()
    out = str(tmp_path / "out")
    X.extract_video(enc, X.FrameFolderReader(root, "b/v7"), str(tmp_path / "f32"))
    big = np.load(str(tmp_path / "f32.npy"))
    n = int((np.abs(big) >= 65520).sum())
    assert n > 0 and np.isfinite(big).all()
    if pack:
        anno = tmp_path / "anno.txt"
        anno.write_text("b/v7 0 6 0\n")
        with pytest.raises(ValueError, match=r"b/v7\.npy: \d+ feature value"):      # (packed launches: the same rows to round-off)
            X.extract_dataset(enc, str(anno), root, out, pack=True, dtype="float16")
    else:
        with pytest.raises(ValueError, match=rf"b/v7\.npy: {n} feature value"):
            X.extract_video(enc, X.FrameFolderReader(root, "b/v7"), os.path.join(out, "b/v7"), dtype="float16")
    assert not os.path.exists(os.path.join(out, "b/v7.npy")) and not os.path.exists(os.path.join(out, "b/v7.npy.tmp"))
    recs = [type("Rec", (), dict(video="b/v7", start_frame=0, end_frame=6, label=0))()]
    with pytest.raises(ValueError, match=r"b/v7: \d+ feature value" if pack else rf"b/v7: {n} feature value"):
        FeatureBank.from_frames(enc, recs, root, bank_dtype="float16", pack=pack)
    torch.cuda.synchronize()


# ====================================================================================================== whole runs
def _run(folders, tag, files=None, bank_dtype=None):
    """Trainer.fit for two steps and Trainer.test of a fresh module (the same seed every time): over the feature files under
    `files`, or from the frame folders with a bank of `bank_dtype`"""
    root, frames, hp = folders
    base = root / tag
    mod, net = build_module(files is not None, base / "save", base / "logs")
    if files is not None:
        dm = AnomalyCLIPDataModule(**hp, frames_root=files)
    else:
        dm = AnomalyCLIPDataModule(**hp, frames_root=frames, load_from_features=False, encoder=net, bank_dtype=bank_dtype)
    net.train()
    torch.manual_seed(77)
    np.random.seed(78)
    losses, batches, step = [], [], mod.train_batch

    def recording(batch, opt, i=0):
        batches.append([t.detach().clone() for pair in batch for t in pair if torch.is_tensor(t)])
        r = step(batch, opt, i)
        losses.append(torch.stack([torch.as_tensor(v).detach().reshape(()) for v in mod.last_losses]).clone())
        return r
    mod.train_batch = recording
    try:
        Trainer(max_epochs=1, limit_train_batches=2, default_root_dir=str(base)).fit(mod, dm)
    finally:
        del mod.train_batch
    metrics = Trainer().test(mod, dm, ckpt_path=str(base / "checkpoints" / "last.ckpt"))
    torch.cuda.synchronize()
    weights = {n: p.detach().clone() for n, p in net.named_parameters()}
    return dict(dm=dm, base=base, losses=losses, batches=batches, weights=weights, metrics=metrics,
                ncentroid=mod.ncentroid.clone())


@pytest.fixture(scope="module")
def runs(folders):
    """float16 files of the three lists (extracted by the module's own encoder), their widened float32 copies, and the runs"""
    root, frames, hp = folders
    _, net = build_module(True, root / "x" / "save", root / "x" / "logs")
    f16, f32 = str(root / "features_f16"), str(root / "features_f32_widened")
    for kind in ("normal", "anomaly", "test"):
        X.extract_dataset(net.eval(), hp[f"annotation_file_{kind}"], frames, f16, dtype="float16")
    for d, _, names in os.walk(f16):
        for n in names:
            h = np.load(os.path.join(d, n))
            assert h.dtype == np.float16
            os.makedirs(os.path.join(f32, os.path.relpath(d, f16)), exist_ok=True)
            np.save(os.path.join(f32, os.path.relpath(d, f16), n), h.astype(np.float32))
    del net
    done = {}

    def get(tag):
        if tag not in done:
            done[tag] = _run(folders, "f16_" + tag, **{"half_files": dict(files=f16), "float_files": dict(files=f32),
                                                        "half_bank": dict(bank_dtype="float16")}[tag])
        return done[tag]
    return get


def _same_run(a, b):
    assert len(a["losses"]) == len(b["losses"]) == 2 and len(a["batches"]) == 2
    for x, y in zip(a["batches"], b["batches"]):
        assert len(x) == len(y) == 4 and all(s.dtype == t.dtype and torch.equal(s, t) for s, t in zip(x, y))
    for x, y in zip(a["losses"], b["losses"]):
        assert torch.isfinite(x).all() and torch.equal(x, y), (x, y)
    assert a["weights"].keys() == b["weights"].keys()
    for n, w in b["weights"].items():
        assert torch.equal(a["weights"][n], w), n
    assert torch.equal(a["ncentroid"], b["ncentroid"])
    for rel in ("save/ncentroid.pt", "save/metrics_0.json", "logs/eval/runs/checkpoints/metrics.json"):
        fa, fb = a["base"] / rel, b["base"] / rel
        if rel.endswith(".pt"):
            assert torch.equal(torch.load(fa), torch.load(fb)), rel
        else:
            assert fa.read_text() == fb.read_text() and "auc_roc" in json.loads(fa.read_text()), rel
    assert a["metrics"] and json.dumps(a["metrics"], sort_keys=True) == json.dumps(b["metrics"], sort_keys=True)


def test_fit_and_test_on_float16_files_equal_the_widened_files(runs):
    """batches, losses, weights, ncentroid and metrics.json: bit for bit those of the float32 files holding the same values"""
    a, b = runs("half_files"), runs("float_files")
    assert a["dm"].bank.dtype == torch.float16 and b["dm"].bank.dtype == torch.float32
    assert a["dm"].bank.nbytes * 2 == b["dm"].bank.nbytes
    assert all(v.dtype == torch.float16 for v in a["dm"].resident_normal_videos())
    _same_run(a, b)


def test_fit_and_test_from_frames_with_a_half_bank(runs):
    """frames mode with bank_dtype="float16" against the float32 bank filled with the rounded rows (the widened files)"""
    a, b = runs("half_bank"), runs("float_files")
    dm = a["dm"]
    assert dm.bank.dtype == torch.float16 and dm._test_bank.dtype == torch.float16 and len(dm.bank) == 6
    assert np.array_equal(dm.bank.bank.cpu().numpy(), runs("half_files")["dm"].bank.bank.cpu().numpy())
    _same_run(a, b)


# ====================================================================================================== what rounding does
# max |difference| of the anomaly scores / of the class probabilities between float32 features and the same features rounded to
# float16 first, on the reference-produced fixtures' inputs (recipes.e2e_inputs of e2e_tiny.npz / e2e_l14.npz).  Recorded ONCE on
# an MI355X with this code (profiles/feature_f16_rounding.json) and not tuned since; the test allows 16 times as much: the error
# is linear in a 2^-11 relative perturbation of the inputs, the margin covers other inputs on the same model.
RECORDED = {"tiny": (3.47793e-05, 9.80496e-05), "l14": (3.18289e-05, 6.92159e-05)}      # (scores, class probabilities)


def rounding_differences(name, golden, prompts_table):
    if name == "tiny":
        from test_gpu_model import build_net
        g = golden("e2e_tiny")
        hc = IW.HeadConfig(num_classes=14, normal_id=7, emb_size=64, heads=2, depth=1)
        net, _, _ = build_net("tiny", hc, "ucf", int(g["seed"]), prompts_table)
        inp = R.e2e_inputs(int(g["seed"]), IW.TINY.embed_dim)
    else:
        from test_gpu_clip_arch import _net
        g = golden("e2e_l14")
        net, _, _ = _net(prompts_table, int(g["seed"]), with_image_encoder=False)
        inp = R.e2e_inputs(int(g["seed"]), 768)
    net.eval()
    feats = inp["test_feats"].to(DEV)
    over = torch.zeros(1, dtype=torch.int64, device=DEV)
    half = ops.cast_rows_f16(feats.view(-1, feats.shape[-1]), over)
    assert int(over) == 0
    rounded = ops.expand_rows_f16(half).view(feats.shape)
    out = []
    with torch.no_grad():
        for x in (feats, rounded):
            sim, sc = net(x, torch.zeros(1000), inp["nc"], 2, True)
            out.append((sc.clone(), ops.class_probs(sim, sc).clone()))
    (sc32, pr32), (sc16, pr16) = out
    assert all(torch.isfinite(t).all() for pair in out for t in pair)
    return (sc16 - sc32).abs().max().item(), (pr16 - pr32).abs().max().item()


@pytest.mark.parametrize("name", ["tiny", "l14"])
def test_scores_from_rounded_features(name, golden, prompts_table):
    d_scores, d_probs = rounding_differences(name, golden, prompts_table)
    print(f"feature_f16 rounding {name}: max |d scores| = {d_scores:.6g}, max |d class probabilities| = {d_probs:.6g}")
    assert d_scores < 16 * RECORDED[name][0] and d_probs < 16 * RECORDED[name][1]
