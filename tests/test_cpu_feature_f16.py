"""CPU-only checks of the half-precision feature files: the new entry points' export and argument checks, FeatureBank's scan of
float16 / mixed / refused files, extract's dtype validation and its overflow refusal with the cast faked.  No kernel runs here."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

NEW = ("acx_cast_rows_f16", "acx_sample_segments_f16", "acx_tile_videos_f16", "acx_expand_rows_f16")


def _aligned(buf, align):
    return (C.addressof(buf) + align - 1) & ~(align - 1)


def test_new_symbols_are_declared_and_exported():
    from anomalyclip_amd import _lib as L
    lib = L.lib()
    for name in NEW:
        assert name in L.declared_symbols(), name
        assert getattr(lib, name) is not None


def test_sample_segments_f16_abi_without_gpu():
    """as test_sample_segments_abi_without_gpu: validates before any launch, names itself in the error"""
    from anomalyclip_amd import _lib as L
    lib = L.lib()
    fn = lib.acx_sample_segments_f16
    bank, out = (C.c_uint16 * 80)(), (C.c_float * 80)()
    row_off, frames, vid, starts = (C.c_int64 * 1)(0), (C.c_int32 * 1)(4), (C.c_int32 * 1)(0), (C.c_int32 * 2)(0, 1)
    pb, po = _aligned(bank, 16), _aligned(out, 16)
    p = [pb] + [C.addressof(x) for x in (row_off, frames, vid, starts)] + [po]
    assert fn(None, *p, 0, 2, 2, 1, 1, 8, None) == 0                                       # B == 0: nothing to do
    assert fn(None, None, *p[1:], 1, 2, 2, 1, 1, 8, None) == -1 and b"null" in lib.acx_last_error(None)
    assert b"acx_sample_segments_f16" in lib.acx_last_error(None)
    for bad in ((-1, 2, 2, 1, 1, 8), (1, 0, 2, 1, 1, 8), (1, 2, 0, 1, 1, 8), (1, 2, 2, 0, 1, 8), (1, 2, 2, 1, 0, 8), (1, 2, 2, 1, 1, 0),
                (1, 2, 2, 1, 1, 6)):
        assert fn(None, *p, *bad, None) == -1, bad
        assert b"acx_sample_segments_f16" in lib.acx_last_error(None)
    # a bank base that is 4-byte but not 8-byte aligned, an out that is 8-byte but not 16-byte aligned
    assert fn(None, pb + 4, *p[1:], 1, 2, 2, 1, 1, 8, None) == -1 and b"acx_sample_segments_f16" in lib.acx_last_error(None)
    assert fn(None, *p[:5], po + 8, 1, 2, 2, 1, 1, 8, None) == -1 and b"aligned" in lib.acx_last_error(None)
    assert fn(None, *p, 1 << 20, 1 << 6, 1 << 6, 1, 1, 8, None) == -1 and b"2^31" in lib.acx_last_error(None)
    if not torch.cuda.is_available():
        assert fn(None, pb + 8, *p[1:], 1, 2, 2, 1, 1, 8, None) in (-3, -2)                # an 8-byte aligned base passes the checks
        assert b"acx_sample_segments_f16" in lib.acx_last_error(None)


def test_tile_videos_f16_abi_without_gpu():
    from anomalyclip_amd import _lib as L
    lib = L.lib()
    fn = lib.acx_tile_videos_f16
    bank, out = (C.c_uint16 * 80)(), (C.c_float * 80)()
    row_off, frames, vid = (C.c_int64 * 1)(0), (C.c_int32 * 1)(4), (C.c_int32 * 1)(0)
    out_off, rows, blk = (C.c_int64 * 1)(0), (C.c_int32 * 1)(4), (C.c_int32 * 1)(0)
    pb, po = _aligned(bank, 16), _aligned(out, 16)
    p = [pb] + [C.addressof(x) for x in (row_off, frames, vid, out_off, rows, blk)] + [po]
    good = (1, 4, 2, 2, 1, 1, 8)                                                           # V, total_rows, N, L, stride, ncrops, D
    assert fn(None, *p, 0, 4, 2, 2, 1, 1, 8, None) == 0                                    # V == 0
    assert fn(None, None, *p[1:], *good, None) == -1 and b"acx_tile_videos_f16: null" in lib.acx_last_error(None)
    for bad in ((-1, 4, 2, 2, 1, 1, 8), (1, 0, 2, 2, 1, 1, 8), (1, 4, 0, 2, 1, 1, 8), (1, 4, 2, 2, 0, 1, 8), (1, 4, 2, 2, 1, 0, 8),
                (1, 4, 2, 2, 1, 1, 6), (1, 6, 2, 2, 1, 1, 8), (1, 1 << 31, 2, 2, 1, 1, 8)):
        assert fn(None, *p, *bad, None) == -1, bad
        assert b"acx_tile_videos_f16" in lib.acx_last_error(None)
    assert fn(None, pb + 4, *p[1:], *good, None) == -1 and b"aligned" in lib.acx_last_error(None)
    if not torch.cuda.is_available():
        assert fn(None, pb + 8, *p[1:], *good, None) in (-3, -2)


def test_cast_and_expand_abi_without_gpu():
    from anomalyclip_amd import _lib as L
    lib = L.lib()
    src, dst, cnt = (C.c_float * 80)(), (C.c_uint16 * 80)(), (C.c_int64 * 2)()
    ps, pd, pc = _aligned(src, 16), _aligned(dst, 16), C.addressof(cnt)
    fn = lib.acx_cast_rows_f16
    assert fn(None, ps, pd, 0, 8, 8, pc, None) == 0                                        # rows == 0: a no-op
    assert fn(None, None, pd, 2, 8, 8, pc, None) == -1 and b"acx_cast_rows_f16: null" in lib.acx_last_error(None)
    assert fn(None, ps, pd, 2, 8, 8, None, None) == -1 and b"acx_cast_rows_f16" in lib.acx_last_error(None)
    for bad in ((-1, 8, 8), (2, 0, 8), (2, 8, 4), (2, 6, 8), (2, 8, 10)):
        assert fn(None, ps, pd, *bad, pc, None) == -1, bad
        assert b"acx_cast_rows_f16" in lib.acx_last_error(None)
    assert fn(None, ps + 4, pd, 2, 8, 8, pc, None) == -1 and b"aligned" in lib.acx_last_error(None)
    assert fn(None, ps, pd + 4, 2, 8, 8, pc, None) == -1 and b"aligned" in lib.acx_last_error(None)
    fn = lib.acx_expand_rows_f16
    assert fn(None, pd, ps, 0, 8, None) == 0
    assert fn(None, None, ps, 2, 8, None) == -1 and b"acx_expand_rows_f16: null" in lib.acx_last_error(None)
    for bad in ((-1, 8), (2, 0), (2, 6)):
        assert fn(None, pd, ps, *bad, None) == -1 and b"acx_expand_rows_f16" in lib.acx_last_error(None), bad
    assert fn(None, pd + 4, ps, 2, 8, None) == -1 and fn(None, pd, ps + 8, 2, 8, None) == -1
    assert b"acx_expand_rows_f16" in lib.acx_last_error(None)
    if not torch.cuda.is_available():
        assert fn(None, pd + 8, ps, 2, 8, None) in (-3, -2)


def test_ops_refuse_other_bank_dtypes():
    """the gathers dispatch on the bank's dtype before anything else: bf16 or float64 is a TypeError, with or without a device"""
    from anomalyclip_amd import ops
    t = torch.zeros(1, dtype=torch.int64)
    for dt in (torch.bfloat16, torch.float64):
        with pytest.raises(TypeError, match="sample_segments.*float32 or float16"):
            ops.sample_segments(torch.zeros(4, 8, dtype=dt), t, t, t, t, 1, 1, 1, 1)
        with pytest.raises(TypeError, match="tile_videos.*float32 or float16"):
            ops.tile_videos(torch.zeros(4, 8, dtype=dt), t, t, [0], [1], 1, 1, 1, 1)


# ====================================================================================================== FeatureBank._scan
def _scan(paths, ncrops=1):
    from anomalyclip_amd.feature_bank import FeatureBank
    return FeatureBank._scan(SimpleNamespace(paths=[str(p) for p in paths], ncrops=ncrops))


def test_scan_accepts_float16_and_refuses_mixed(tmp_path):
    rng = np.random.default_rng(0)
    for i, T in enumerate((5, 9, 2)):
        a = rng.standard_normal((T, 8)).astype(np.float32)
        np.save(tmp_path / f"h{i}.npy", a.astype(np.float16))
        np.save(tmp_path / f"f{i}.npy", a)
    halves, floats = [tmp_path / f"h{i}.npy" for i in range(3)], [tmp_path / f"f{i}.npy" for i in range(3)]
    assert _scan(halves) == ([5, 9, 2], 8, torch.float16)
    assert _scan(floats) == ([5, 9, 2], 8, torch.float32)
    with pytest.raises(ValueError, match=r"f2\.npy.*float32.*float16"):
        _scan([halves[0], halves[1], floats[2]])                       # names the first file that differs
    with pytest.raises(ValueError, match=r"h1\.npy"):
        _scan([floats[0], halves[1], halves[2]])


def test_scan_still_refuses_float64_fortran_and_1d(tmp_path):
    np.save(tmp_path / "f64.npy", np.zeros((3, 8)))
    np.save(tmp_path / "fortran.npy", np.asfortranarray(np.zeros((3, 8), np.float16)))
    np.save(tmp_path / "d1.npy", np.zeros(8, np.float16))
    np.save(tmp_path / "w6.npy", np.zeros((3, 6), np.float16))
    for name in ("f64", "fortran", "d1", "w6"):
        with pytest.raises(ValueError, match=name + r"\.npy"):
            _scan([tmp_path / f"{name}.npy"])
    np.save(tmp_path / "ok.npy", np.zeros((3, 8), np.float16))
    with pytest.raises(ValueError, match="ncrops"):
        _scan([tmp_path / "ok.npy"], ncrops=2)


def test_bank_dtype_key_is_validated(tmp_path):
    from anomalyclip_amd.datamodule import AnomalyCLIPDataModule
    from anomalyclip_amd.feature_bank import FeatureBank, check_bank_dtype
    import inspect
    assert check_bank_dtype("float16") == torch.float16 and check_bank_dtype("float32") == torch.float32
    assert inspect.signature(FeatureBank.from_frames).parameters["bank_dtype"].default == "float32"
    assert inspect.signature(AnomalyCLIPDataModule.__init__).parameters["bank_dtype"].default == "float32"
    enc = SimpleNamespace(output_dim=32)
    rec = [SimpleNamespace(video="v", start_frame=0, end_frame=3, label=0)]
    with pytest.raises(ValueError, match="bank_dtype"):
        FeatureBank.from_frames(enc, rec, str(tmp_path), max_bytes=1 << 30, bank_dtype="bfloat16")
    with pytest.raises(ValueError, match="bank_dtype"):
        AnomalyCLIPDataModule(bank_dtype="half")
    # the size check counts two bytes per element
    with pytest.raises(ValueError, match=r"need 256 bytes.*float16"):
        FeatureBank.from_frames(enc, rec, str(tmp_path), max_bytes=255, bank_dtype="float16")


# ====================================================================================================== extract
def test_extract_dtype_is_validated_before_any_file_is_opened(tmp_path, capsys):
    from anomalyclip_amd import extract as X

    class Untouchable:                                    # any use of the frames or the encoder fails the test
        def __getattr__(self, name):
            raise AssertionError(f"touched .{name}")

        def __len__(self):
            raise AssertionError("touched len()")

    with pytest.raises(ValueError, match="dtype='bogus'"):
        X.extract_video(Untouchable(), Untouchable(), str(tmp_path / "x"), dtype="bogus")
    with pytest.raises(ValueError, match="dtype='float64'"):
        X.extract_dataset(Untouchable(), str(tmp_path / "no_such_list.txt"), str(tmp_path), str(tmp_path / "out"), dtype="float64")
    with pytest.raises(ValueError, match="dtype"):
        X.extract_dataset(Untouchable(), None, str(tmp_path), str(tmp_path / "out"), pack=True, dtype=None)
    assert not os.listdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        X.parse_args(["--arch", "tiny", "--weights", "w", "--frames-root", "f", "--out-root", "o", "--dtype", "bogus"])
    assert e.value.code == 2 and "--dtype" in capsys.readouterr().err
    assert X._parser().parse_args(["--arch", "tiny", "--weights", "w", "--frames-root", "f", "--out-root", "o"]).dtype == "float32"


def test_is_complete_and_write_features_know_both_dtypes(tmp_path):
    from anomalyclip_amd import extract as X
    rows = np.random.default_rng(1).standard_normal((6, 8)).astype(np.float32)
    out = str(tmp_path / "v")
    p = X.write_features(out, rows.astype(np.float16))
    got = np.load(p)
    assert got.dtype == np.float16 and np.array_equal(got, rows.astype(np.float16)) and not os.path.exists(p + ".tmp")
    with open(p, "rb") as fh:
        from anomalyclip_amd.feature_stream import FeatureStream
        shape, fortran, dtype = FeatureStream._npy_header(fh)
    assert tuple(shape) == (6, 8) and not fortran and dtype == np.dtype("<f2")
    # a present file of the other dtype is never kept: it is not complete, so the extractor rewrites it
    assert X.is_complete(out, rows.shape, "float16") and not X.is_complete(out, rows.shape) and not X.is_complete(out, rows.shape, "float32")
    X.write_features(out, rows)
    assert np.load(p).dtype == np.float32
    assert X.is_complete(out, rows.shape) and not X.is_complete(out, rows.shape, "float16")


def test_overflow_refusal_leaves_no_file(tmp_path):
    """the counter a video's casts added to is looked at before the write: by extract's own check and by the writer thread"""
    from anomalyclip_amd import extract as X
    out = str(tmp_path / "a" / "v")
    X.check_overflow(None, out)
    X.check_overflow(torch.zeros(1, dtype=torch.int64), out)
    with pytest.raises(ValueError, match=r"v\.npy: 3 feature value\(s\) do not fit float16"):
        X.check_overflow(torch.tensor([3]), out)
    rows = np.ones((4, 8), np.float16)
    done = []
    w = X.FeatureWriter(3, done=done.append)
    for _ in range(3):                                                 # the three places first: acquire() re-raises a kept error, and
        w.acquire()                                                    # whether the thread has met the bad job by then is a race
    w.submit(None, rows, str(tmp_path / "good"), 0, torch.zeros(1, dtype=torch.int64))
    w.submit(None, rows, out, 1, torch.tensor([2]))
    w.submit(None, rows, str(tmp_path / "behind"), 2, None)            # behind a failure: dropped unwritten
    with pytest.raises(ValueError, match=r"a/v\.npy: 2 feature value"):
        w.close()
    assert done == [0] and np.load(tmp_path / "good.npy").dtype == np.float16
    assert not os.path.exists(out + ".npy") and not os.path.exists(out + ".npy.tmp") and not os.path.exists(tmp_path / "behind.npy")


def test_extract_video_overflow_with_the_cast_faked(tmp_path, monkeypatch):
    """extract_video(dtype="float16") with the encode loop and the cast replaced by host stand-ins: a counted overflow raises and
    nothing lies under the final name; without one the file is the rounded rows"""
    from anomalyclip_amd import extract as X
    from anomalyclip_amd import ops
    rows = torch.from_numpy(np.random.default_rng(2).standard_normal((6, 8)).astype(np.float32))
    rows[4, 3] = 70000.0
    enc = SimpleNamespace(output_dim=8, training=False, modules=lambda: [], parameters=lambda: iter([torch.zeros(1)]))

    def fake_cast(src, overflow, out=None):
        h = src.to(torch.float16)
        overflow += int((torch.isinf(h) & torch.isfinite(src)).sum())
        return h

    monkeypatch.setattr(X, "check_encoder", lambda e: None)
    monkeypatch.setattr(X, "encode_video", lambda e, r, n, s: iter([(0, rows[:4]), (4, rows[4:])]))
    monkeypatch.setattr(ops, "cast_rows_f16", fake_cast)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: SimpleNamespace(synchronize=lambda: None))
    frames = np.zeros((6, 4, 4, 3), np.uint8)
    with pytest.raises(ValueError, match=r"bad\.npy: 1 feature value"):
        X.extract_video(enc, frames, str(tmp_path / "bad"), dtype="float16")
    assert not os.listdir(tmp_path)
    rows[4, 3] = 65519.0                                                # the largest float that still rounds to 65504
    r = X.extract_video(enc, frames, str(tmp_path / "good"), dtype="float16")
    assert r == {"written": True, "frames": 6, "rows": 6}
    got = np.load(tmp_path / "good.npy")
    assert got.dtype == np.float16 and np.array_equal(got, rows.numpy().astype(np.float16))
    assert X.extract_video(enc, frames, str(tmp_path / "good"), dtype="float16")["written"] is False       # complete: kept
    assert X.extract_video(enc, frames, str(tmp_path / "good"))["written"] is True                         # other dtype: rewritten
    assert np.load(tmp_path / "good.npy").dtype == np.float32
