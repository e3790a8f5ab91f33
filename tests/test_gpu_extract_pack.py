"""-m gpu: packed extraction (extract.encode_videos, extract_dataset(pack=True), FeatureBank.from_frames(pack=True), `--pack`)
against the unpacked run of the same folders: the tiny ViT at chunk 16 over five folders of 1, 7, 16, 23 and 40 JPEG frames of two
sizes, one of them progressive (Pillow's, in the middle of a packed launch), for 1 and 5 crops and the three decoders.

The gates ("Packed extraction"): a packed file has the unpacked file's shape and dtype and its rows within
relerr 1e-5 -- the bound test_resnet_bf16x6_identical_frames_in_one_launch holds one module to at two batch sizes; two packed
runs write the same bytes.  Whether a packed file is byte-identical to the unpacked one is printed, not asserted."""
import math
import os
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jpeg_restated as JR
from anomalyclip_amd import extract as X
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd import jpeg as J
from anomalyclip_amd.feature_bank import FeatureBank

DEV = "cuda"
GATE = 1e-5
CHUNK = 16
LENGTHS = [1, 7, 16, 23, 40]
SIZES = [(48, 64), (60, 80)]
PROGRESSIVE = (3, 10)                  # video 3, frame 10: frame 34 of the run, inside launch 2 at one crop


def relerr(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _write_folder(folder, T, hw, seed, progressive=()):
    os.makedirs(folder, exist_ok=True)
    for t in range(T):
        kw = dict(progressive=True) if t in progressive else {}
        with open(os.path.join(folder, f"{t:06d}.jpg"), "wb") as fh:
            fh.write(JR.save_jpeg(JR.make_image(hw[0], hw[1], 25, seed=seed * 100 + t), 60 + 5 * (t % 4), 2, **kw))


@pytest.fixture(scope="module")
def frames_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("pack_frames"))
    for v, T in enumerate(LENGTHS):
        _write_folder(os.path.join(root, f"v{v}"), T, SIZES[v % 2], v, (PROGRESSIVE[1],) if v == PROGRESSIVE[0] else ())
    return root


@pytest.fixture(scope="module")
def tiny():
    enc = X.build_image_encoder("tiny", "f32", chunk=CHUNK)
    enc.load_state_dict(IW.init_vit_state_dict(IW.TINY, 13, prefix=""), strict=True)
    return enc.to(DEV).eval()


class _Calls:
    """counts the encoder's forward calls and keeps every frame reader extract_dataset makes"""

    def __init__(self, enc, monkeypatch):
        self.n, self.readers = 0, []
        fwd, make = enc.forward, J.make_reader

        def forward(x):
            self.n += 1
            assert x.shape[0] <= enc.chunk
            return fwd(x)

        def make_reader(*a, **k):
            self.readers.append(make(*a, **k))
            return self.readers[-1]

        monkeypatch.setattr(enc, "forward", forward, raising=False)
        monkeypatch.setattr(J, "make_reader", make_reader)

    def take(self):
        n, fb = self.n, sum(getattr(r, "fallbacks", 0) for r in self.readers)
        self.n, self.readers = 0, []
        return n, fb


def _run(enc, root, out, ncrops, decode, pack, **kw):
    lines = []
    counts = X.extract_dataset(enc, None, root, out, ncrops=ncrops, decode=decode, pack=pack, log=lines.append, **kw)
    return counts, lines


def _files(out):
    return {v: np.load(os.path.join(out, f"v{v}.npy"), allow_pickle=False) for v in range(len(LENGTHS))}


_unpacked = {}


def _reference(enc, root, tmp_factory, ncrops, decode, calls):
    """the unpacked run of (ncrops, decode): made once, shared, never changed"""
    if (ncrops, decode) not in _unpacked:
        out = str(tmp_factory.mktemp(f"unpacked_{ncrops}_{decode}"))
        counts, lines = _run(enc, root, out, ncrops, decode, False)
        n, fb = calls.take()
        files = _files(out)
        _unpacked[(ncrops, decode)] = (counts, [l.replace(out, "<out>") for l in lines], n, fb, files)
    return _unpacked[(ncrops, decode)]


@pytest.mark.parametrize("decode", ["pil", "gpu", "gpu_entropy"])
@pytest.mark.parametrize("ncrops", [1, 5])
def test_packed_files_against_unpacked(tmp_path, tmp_path_factory, monkeypatch, frames_root, tiny, ncrops, decode):
    calls = _Calls(tiny, monkeypatch)
    nb = X.batch_frames(tiny, ncrops)
    assert nb == CHUNK // ncrops
    counts0, lines0, n0, fb0, ref = _reference(tiny, frames_root, tmp_path_factory, ncrops, decode, calls)
    want = {"written": 5, "skipped": 0, "frames": sum(LENGTHS), "rows": sum(LENGTHS) * ncrops}
    assert counts0 == want and n0 == sum(math.ceil(T / nb) for T in LENGTHS)
    start = threading.active_count()
    out = str(tmp_path / "packed")
    counts, lines = _run(tiny, frames_root, out, ncrops, decode, True)
    n, fb = calls.take()
    plan = X.plan_launches(LENGTHS, ncrops, CHUNK)
    assert any(PROGRESSIVE[0] == v and i0 <= PROGRESSIVE[1] < i1 and (len(launch) > 1 or ncrops == 5)
               for launch in plan for v, i0, i1 in launch)
    assert n == len(plan) < n0                                                # one encoder call per planned launch
    assert counts == want and [l.replace(out, "<out>") for l in lines] == lines0
    assert lines0 == [f"wrote {os.path.join('<out>', f'v{v}.npy')}  [{T * ncrops} rows]" for v, T in enumerate(LENGTHS)]
    assert fb == fb0 == (0 if decode == "pil" else 1)                          # the progressive file, and only it, is Pillow's
    assert threading.active_count() == start
    assert not [f for f in os.listdir(out) if f.endswith(".tmp")]
    got = _files(out)
    same = []
    for v, T in enumerate(LENGTHS):
        assert got[v].shape == ref[v].shape == (T * ncrops, 128) and got[v].dtype == ref[v].dtype == np.float32
        e = relerr(got[v], ref[v])
        same.append(got[v].tobytes() == ref[v].tobytes())
        print(f"tiny f32, {ncrops} crop(s), {decode}: v{v} relerr {e:.3g}, byte-identical {same[-1]}")
        assert e <= GATE
    print(f"PACKED-VS-UNPACKED tiny f32 ncrops={ncrops} decode={decode}: byte-identical files {sum(same)} of {len(same)}")


@pytest.mark.parametrize("decode", ["pil", "gpu_entropy"])
def test_two_packed_runs_write_the_same_bytes(tmp_path, frames_root, tiny, decode):
    for k in range(2):
        assert X.extract_dataset(tiny, None, frames_root, str(tmp_path / str(k)), ncrops=5, decode=decode, pack=True)["written"] == 5
    a, b = _files(str(tmp_path / "0")), _files(str(tmp_path / "1"))
    for v in a:
        assert a[v].tobytes() == b[v].tobytes(), v


def test_packed_run_skips_complete_files(tmp_path, monkeypatch, frames_root, tiny):
    calls = _Calls(tiny, monkeypatch)
    out = str(tmp_path / "o")
    anno = tmp_path / "anno.txt"
    anno.write_text("".join(f"v{v} 0 {T - 1} 0\n" for v, T in enumerate(LENGTHS)))
    first = X.extract_dataset(tiny, str(anno), frames_root, out, ncrops=5, pack=True)
    assert first["written"] == 5 and calls.take()[0] == len(X.plan_launches(LENGTHS, 5, CHUNK))
    paths = [os.path.join(out, f"v{v}.npy") for v in range(5)]
    keep = [np.load(p) for p in paths]
    for p in paths:
        os.utime(p, ns=(10 ** 18, 10 ** 18))
    lines = []
    again = X.extract_dataset(tiny, str(anno), frames_root, out, ncrops=5, pack=True, log=lines.append)
    assert again == {"written": 0, "skipped": 5, "frames": 0, "rows": 0} and calls.take()[0] == 0      # nothing launched
    assert lines == [f"kept  {p}  [{T * 5} rows]" for p, T in zip(paths, LENGTHS)]
    assert all(os.stat(p).st_mtime_ns == 10 ** 18 for p in paths)
    os.remove(paths[3])
    lines = []
    third = X.extract_dataset(tiny, str(anno), frames_root, out, ncrops=5, pack=True, log=lines.append)
    assert third == {"written": 1, "skipped": 4, "frames": 23, "rows": 115}
    assert calls.take()[0] == len(X.plan_launches([23], 5, CHUNK)) == 8                              # only that video's launches
    assert [l[:5] for l in lines] == ["kept ", "kept ", "kept ", "wrote", "kept "]
    assert [os.stat(p).st_mtime_ns == 10 ** 18 for p in paths] == [True, True, True, False, True]
    assert relerr(np.load(paths[3]), keep[3]) <= GATE                            # (alone in its launches now: another packing)
    fresh = X.extract_dataset(tiny, str(anno), frames_root, out, ncrops=5, pack=True, overwrite=True, max_inflight=1)
    assert fresh["written"] == 5
    for p, k in zip(paths, keep):
        assert np.load(p).tobytes() == k.tobytes()                               # the first run's packing again: its bytes


def test_a_missing_frame_ends_the_packed_run_cleanly(tmp_path, frames_root, tiny):
    """video 3's annotation row names a frame past its folder's end: the error reaches the caller, the files of the videos finished
    before it stay and are whole, no .tmp is left and no thread outlives the call"""
    out = str(tmp_path / "o")
    anno = tmp_path / "anno.txt"
    ends = [T - 1 for T in LENGTHS]
    ends[3] += 2
    anno.write_text("".join(f"v{v} 0 {e} 0\n" for v, e in enumerate(ends)))
    start = threading.active_count()
    with pytest.raises(FileNotFoundError, match="000023.jpg"):
        X.extract_dataset(tiny, str(anno), frames_root, out, ncrops=1, pack=True)
    assert threading.active_count() == start
    assert not [f for f in os.listdir(out) if f.endswith(".tmp")]
    assert X.is_complete(os.path.join(out, "v0"), (1, 128)) and X.is_complete(os.path.join(out, "v1"), (7, 128))
    assert not os.path.exists(os.path.join(out, "v3.npy")) and not os.path.exists(os.path.join(out, "v4.npy"))


def test_encode_videos_pieces_and_open_readers(frames_root, tiny):
    """the generator's protocol: (key, row0, rows) per piece in plan order; the readers are opened lazily, at most `lookahead`
    ahead of the one being decoded"""
    opened = []

    def readers():
        for v in range(len(LENGTHS)):
            opened.append(v)
            yield f"k{v}", X.FrameFolderReader(frames_root, f"v{v}")

    got = []
    for key, r0, rows in X.encode_videos(tiny, readers(), ncrops=5, lookahead=1, decode_threads=3):
        assert rows.is_cuda and rows.dtype == torch.float32 and rows.shape[1] == 128
        v = int(key[1:])
        if not got:
            assert len(opened) <= 3                                             # v0 in use, one ahead, one being opened
        if v == 3:
            assert max(opened) <= 4
        got.append((v, r0 // 5, (r0 + rows.shape[0]) // 5))
    assert got == [p for launch in X.plan_launches(LENGTHS, 5, CHUNK) for p in launch]


@pytest.mark.parametrize("precision", ["bf16x6", "f32"])
def test_packed_rn50(tmp_path, precision):
    """RN50 at 224 pixels, three folders of two frames, four frames per launch: packed 4 + 2 against unpacked 2 + 2 + 2"""
    with torch.device(DEV):
        enc = X.build_image_encoder("RN50", precision, chunk=4)
    enc.load_state_dict(IW.init_resnet_state_dict(IW.RN50, 17, prefix=""), strict=True)
    enc.eval()
    root = str(tmp_path / "frames")
    for v in range(3):
        _write_folder(os.path.join(root, f"v{v}"), 2, SIZES[v % 2], 40 + v)
    a = X.extract_dataset(enc, None, root, str(tmp_path / "a"), pack=False)
    b = X.extract_dataset(enc, None, root, str(tmp_path / "b"), pack=True)
    assert a == b == {"written": 3, "skipped": 0, "frames": 6, "rows": 6}
    same = 0
    for v in range(3):
        fa, fb = np.load(tmp_path / "a" / f"v{v}.npy"), np.load(tmp_path / "b" / f"v{v}.npy")
        assert fa.shape == fb.shape == (2, enc.output_dim) and fa.dtype == fb.dtype == np.float32 and np.isfinite(fb).all()
        e = relerr(fb, fa)
        same += fa.tobytes() == fb.tobytes()
        print(f"RN50 {precision}: v{v} relerr {e:.3g}")
        assert e <= GATE
    print(f"PACKED-VS-UNPACKED RN50 {precision} ncrops=1 decode=pil: byte-identical files {same} of 3")


@pytest.mark.parametrize("decode", ["pil", "gpu"])
def test_bank_from_frames_packed(frames_root, tiny, decode):
    recs = [SimpleNamespace(video=f"v{v}", start_frame=0, end_frame=T - 1, label=v % 3) for v, T in enumerate(LENGTHS)]
    recs[4] = SimpleNamespace(video="v4", start_frame=3, end_frame=30, label=2)
    lines = []
    plain = FeatureBank.from_frames(tiny, recs, frames_root, ncrops=5, decode=decode)
    packed = FeatureBank.from_frames(tiny, recs, frames_root, ncrops=5, decode=decode, pack=True, log=lines.append)
    assert packed.bank.shape == plain.bank.shape == ((1 + 7 + 16 + 23 + 28) * 5, 128)
    assert np.array_equal(packed.offsets, plain.offsets) and packed.num_frames == plain.num_frames and packed.paths == plain.paths
    for name in ("row_off", "frames", "labels"):
        assert torch.equal(getattr(packed, name), getattr(plain, name)), name
    assert len(lines) == 5 and lines[0].startswith("encoded ")
    e = relerr(packed.bank, plain.bank)
    print(f"PACKED-VS-UNPACKED bank tiny f32 ncrops=5 decode={decode}: relerr {e:.3g}, identical {torch.equal(packed.bank, plain.bank)}")
    assert e <= GATE


def test_command_line_pack(tmp_path, frames_root, tiny, capsys):
    import json
    w = str(tmp_path / "enc.pt")
    torch.save({k: v.cpu() for k, v in tiny.state_dict().items()}, w)
    out = str(tmp_path / "cli")
    assert X.main(["--arch", "tiny", "--weights", w, "--frames-root", frames_root, "--out-root", out, "--ncrops", "5",
                   "--precision", "f32", "--decode", "gpu", "--pack"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == {"written": 5, "skipped": 0, "frames": 87, "rows": 435}
    for v, T in enumerate(LENGTHS):
        a = np.load(os.path.join(out, f"v{v}.npy"))
        assert a.shape == (T * 5, 128) and a.dtype == np.float32 and np.isfinite(a).all()
