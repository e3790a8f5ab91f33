"""CPU-only checks of training from frame folders (`data.load_from_features: false`): what the datamodule accepts and refuses, the
size of a bank that is filled from frames and its memory refusal (with a stub encoder: nothing is decoded, no device is touched),
the index rule of the test-mode tile kernel against feature_index, and acx_tile_videos' argument checks.  No kernel runs here."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from anomalyclip_amd import feature_index as FI

KW = dict(frames_root="/f", annotation_file_normal="n", annotation_file_anomaly="a", annotation_file_test="t",
          annotation_file_temporal_test=None, labels_file=None, normal_id=7, num_classes=14)


def test_frames_mode_needs_an_encoder():
    from anomalyclip_amd.datamodule import AnomalyCLIPDataModule
    with pytest.raises(ValueError, match=r"load_from_features.*encoder="):
        AnomalyCLIPDataModule(**KW, load_from_features=False)
    with pytest.raises(ValueError, match=r"load_from_features.*encoder="):
        AnomalyCLIPDataModule(**KW, load_from_features=False, encoder=None)


def test_frames_mode_accepts_a_net_or_its_image_encoder():
    from anomalyclip_amd.datamodule import AnomalyCLIPDataModule
    enc = SimpleNamespace(output_dim=512)
    for given in (enc, SimpleNamespace(image_encoder=enc)):
        dm = AnomalyCLIPDataModule(**KW, load_from_features=False, encoder=given)
        assert dm.encoder is enc and dm.yields_features is True and dm.hparams.load_from_features is False
        assert "encoder" not in dm.hparams and dm.bank is None and dm.resident_normal_videos() is None
    with pytest.raises(ValueError, match="ncrops=3"):
        AnomalyCLIPDataModule(**KW, load_from_features=False, encoder=enc, ncrops=3)
    # features mode: as before; an encoder given beside feature files is not used
    dm = AnomalyCLIPDataModule(**KW, encoder=enc)
    assert dm.encoder is None and dm.yields_features is True


def _records(spans):
    return [SimpleNamespace(video=f"v{i}", start_frame=a, end_frame=b, label=i % 3) for i, (a, b) in enumerate(spans)]


@pytest.mark.parametrize("ncrops", [1, 5, 10])
def test_bank_from_frames_is_sized_before_any_frame_is_opened(tmp_path, ncrops, monkeypatch):
    """three rows of 20, 1 and 41 frames (end inclusive, one row starting past frame 0): 62 * ncrops rows of 640 floats.  The
    folders do not exist and the reader is booby-trapped: the refusal comes from the arithmetic alone."""
    from anomalyclip_amd import extract as X
    from anomalyclip_amd.feature_bank import FeatureBank

    def opened(*a, **k):
        raise AssertionError("a frame folder was opened before the size check")
    monkeypatch.setattr(X, "FrameFolderReader", opened)
    enc = SimpleNamespace(output_dim=640)
    need = 62 * ncrops * 640 * 4
    with pytest.raises(ValueError, match=rf"need {need} bytes.* {need - 1} bytes are available.*anomalyclip_amd\.extract"):
        FeatureBank.from_frames(enc, _records([(0, 19), (7, 7), (10, 50)]), str(tmp_path / "nowhere"), ncrops=ncrops, max_bytes=need - 1)
    # exactly enough passes the size check and then asks the stub for what only a real encoder has
    with pytest.raises(AttributeError):
        FeatureBank.from_frames(enc, _records([(0, 19), (7, 7), (10, 50)]), str(tmp_path / "nowhere"), ncrops=ncrops, max_bytes=need)


def test_bank_from_frames_refuses_bad_rows_and_crops(tmp_path):
    from anomalyclip_amd.feature_bank import FeatureBank
    enc = SimpleNamespace(output_dim=512)
    with pytest.raises(ValueError, match="ncrops = 2"):
        FeatureBank.from_frames(enc, _records([(0, 3)]), str(tmp_path), ncrops=2, max_bytes=1 << 30)
    with pytest.raises(ValueError, match="v1.*0 frames"):
        FeatureBank.from_frames(enc, _records([(0, 3), (5, 4)]), str(tmp_path), max_bytes=1 << 30)
    with pytest.raises(ValueError, match="no videos"):
        FeatureBank.from_frames(enc, [], str(tmp_path), max_bytes=1 << 30)
    with pytest.raises(ValueError, match="multiple of 4"):
        FeatureBank.from_frames(SimpleNamespace(output_dim=30), _records([(0, 3)]), str(tmp_path), max_bytes=1 << 30)


@pytest.mark.parametrize("N,L", [(32, 16), (4, 2)])
@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("T", [1, 5, 15, 16, 17, 511, 512, 513, 1025])
def test_tile_row_is_frame_r_stride_mod_T(T, stride, N, L):
    """the kernel's rule against the reference's tables: rows = N * L * S, row r = frame (r * stride) mod T"""
    starts, S = FI.test_start_indices(T, N, L, stride)
    table = FI.frame_index_table(starts, L, stride, T)
    assert S == -(-T // (N * L * stride)) and table.shape == (N * L * S,)
    assert np.array_equal(table, (np.arange(N * L * S, dtype=np.int64) * stride) % T)


def test_bank_tile_geometry_without_a_device():
    from anomalyclip_amd.feature_bank import BankTile
    bank = SimpleNamespace(file_frames=[5, 513, 1025], ncrops=5, D=128)
    for v, S in enumerate((1, 2, 3)):
        t = BankTile(bank, v, 32, 16, 1)
        assert (t.S, t.rows, tuple(t.shape), t.dim()) == (S, 512 * S, (1, 5, 512 * S, 128), 4)
    assert BankTile(bank, 2, 4, 2, 3).S == 43                    # ceil(1025 / 24)


def test_tile_videos_abi_without_gpu():
    """exported, validates its arguments before any launch, and fails with a HIP error code (no abort) without a device"""
    from anomalyclip_amd import _lib as L
    lib = L.lib()
    assert "acx_tile_videos" in L.declared_symbols()
    fn = lib.acx_tile_videos
    bank, out = (C.c_float * 72)(), (C.c_float * 72)()
    row_off, frames, vid = (C.c_int64 * 1)(0), (C.c_int32 * 1)(4), (C.c_int32 * 1)(0)
    out_off, rows, blk = (C.c_int64 * 1)(0), (C.c_int32 * 1)(4), (C.c_int32 * 1)(0)
    p = [C.addressof(x) for x in (bank, row_off, frames, vid, out_off, rows, blk, out)]
    p[0], p[7] = (p[0] + 15) & ~15, (p[7] + 15) & ~15
    good = (1, 4, 2, 2, 1, 1, 8)                                  # V, total_rows, N, L, stride, ncrops, D
    assert fn(None, *p, 0, 4, 2, 2, 1, 1, 8, None) == 0           # V == 0: nothing to do
    for k in range(8):
        q = list(p)
        q[k] = None
        assert fn(None, *q, *good, None) == -1 and b"null" in lib.acx_last_error(None), k
    for bad in ((-1, 4, 2, 2, 1, 1, 8), (1, 0, 2, 2, 1, 1, 8), (1, 4, 0, 2, 1, 1, 8), (1, 4, 2, 0, 1, 1, 8), (1, 4, 2, 2, 0, 1, 8),
                (1, 4, 2, 2, 1, 0, 8), (1, 4, 2, 2, 1, 1, 0), (1, 4, 2, 2, 1, 1, 6), (1, 6, 2, 2, 1, 1, 8),
                (1, 1 << 31, 2, 2, 1, 1, 8), (1, 1 << 30, 2, 2, 2, 1, 8)):
        assert fn(None, *p, *bad, None) == -1, bad                # ACX_E_BADARG
        assert b"acx_tile_videos" in lib.acx_last_error(None)
    q = list(p)
    q[7] += 4                                                     # a misaligned out
    assert fn(None, *q, *good, None) == -1 and b"aligned" in lib.acx_last_error(None)
    if not torch.cuda.is_available():
        assert fn(None, *p, *good, None) in (-3, -2)              # ACX_E_HIP / ACX_E_UNSUPPORTED
        assert b"acx_tile_videos" in lib.acx_last_error(None)
