"""Feature files from frame folders: `<frames_root>/<video>/{:06d}.jpg` -> `<out_root>/<video>.npy`, float32 `[T * ncrops, D]`,
row `t * ncrops + c` = crop c of frame t -- the files `feature_stream.py`, `feature_index.py` and the reference's
`data.load_from_features=True` route read (feature_dataset.py:326,347).

Per video: frames are decoded on a thread pool into two pinned uint8 buffers in rotation (the reference's
`Image.open(...).convert("RGB")`, video_dataset.py:204), copied to the device on a side stream, cropped and normalised by ONE
`preprocess_crops` call per batch, encoded by the CLIP image encoder at its own precision, and the rows come back asynchronously
into a pinned `[T * ncrops, D]` buffer.  A batch is `max(1, chunk // ncrops)` frames, i.e. one encoder launch of at most `chunk`
rows; decoding batch k + 1 overlaps the GPU's work on batch k.  `decode="gpu"` (`--decode gpu`) leaves only the Huffman decoding of
baseline JPEG files on the host and reconstructs the frames on the device (anomalyclip_amd/jpeg.py): the same bytes, the same files.

`pack=True` (`--pack`) is for datasets of many short clips: `encode_videos` cuts ALL videos' frames into full launches
(`plan_launches`), decodes launch k + 1 while launch k is encoded whichever videos they belong to, and `extract_dataset` has a
`FeatureWriter` thread write the files behind the encode loop.  Off by default; with it off every call runs the per-video loop above.

`dtype="float16"` (`--dtype float16`) writes half-precision files (numpy's '<f2', the same shape): every block of encoder rows is
rounded on the device (ops.cast_rows_f16: to nearest even, as numpy's astype rounds) before it is copied back, so the copy, the
pinned buffers and the writer move half the bytes.  A feature that no half holds (|x| >= 65520) is a ValueError naming the video,
and no file is left under the final name.  A present file of the OTHER dtype never counts as complete: it is rewritten.

    python -m anomalyclip_amd.extract --arch ViT-B/16 --weights last.ckpt --frames-root frames --out-root features --ncrops 5
"""
from __future__ import annotations

import os
import queue
import re
import sys
import threading
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from typing import Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

TEMPLATE = "{:06d}.jpg"                # the reference's default imagefile_template (video_dataset.py:171)
MAX_DECODE_THREADS = 16                # the decode pool never grows beyond this, whatever the machine has
DTYPES = ("float32", "float16")        # what a feature file may hold


def check_dtype(dtype) -> str:
    """dtype= of extract_video / extract_dataset: "float32" or "float16" """
    if dtype not in DTYPES:
        raise ValueError(f"dtype={dtype!r}: feature files are written as 'float32' or 'float16'")
    return dtype


# ---------------------------------------------------------------------------------------------------------------- frames
def read_annotations(path: str) -> List[Tuple[str, int, int]]:
    """rows `path start end label...` (video_dataset.py:33-38: four or more fields) -> [(path, start, end)], end inclusive"""
    out = []
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            row = line.strip().split()
            if not row:
                continue
            if len(row) < 4:
                raise ValueError(f"{path}:{n}: expected `path start end label...`, got {line.strip()!r}")
            out.append((row[0], int(row[1]), int(row[2])))
    return out


def _template_regex(template: str):
    """a regex whose group 1 is the frame number of a file name made by `template`"""
    m = re.fullmatch(r"(.*)\{(?::0?(\d*)d?)?\}(.*)", template)
    if m is None:
        raise ValueError(f"imagefile template {template!r} needs exactly one integer field, like '{{:06d}}.jpg'")
    return re.compile(re.escape(m.group(1)) + r"(\d+)" + re.escape(m.group(3)))


class FrameFolderReader:
    """The frames `start ... end` (inclusive) of `<frames_root>/<video>/<template>`; without a range, every file of the folder
    that matches the template, in frame order.  `batches(n)` decodes n frames at a time on a thread pool into two uint8 buffers
    in rotation (pinned when a GPU is there), one batch ahead of its consumer."""

    def __init__(self, frames_root: str, video: str, start: Optional[int] = None, end: Optional[int] = None,
                 template: str = TEMPLATE, threads: int = 8, pinned: Optional[bool] = None):
        self.dir = os.path.join(frames_root, video)
        self.template = template
        if (start is None) != (end is None):
            raise ValueError("start and end go together")
        if start is None:
            rx = _template_regex(template)
            idx = []
            for name in os.listdir(self.dir):
                m = rx.fullmatch(name)
                if m and template.format(int(m.group(1))) == name:
                    idx.append(int(m.group(1)))
            self.indices = sorted(idx)
        else:
            self.indices = list(range(int(start), int(end) + 1))
        if not self.indices:
            raise ValueError(f"{self.dir}: no frames ({template})")
        self._init_reader(threads, pinned)

    def _init_reader(self, threads: int, pinned: Optional[bool]):
        """the reader's state beside `dir`, `template` and `indices` (also for a reader made from another's frames)"""
        self.threads = max(1, min(int(threads), MAX_DECODE_THREADS))
        self.pinned = torch.cuda.is_available() if pinned is None else bool(pinned)
        self._buf = [None, None]
        self.copied = [None, None]      # per slot: the consumer's event after the copy that READ the buffer (set by the consumer)
        self._pool = None
        self._borrowed = False
        self._size = None

    def __len__(self) -> int:
        return len(self.indices)

    def path(self, i: int) -> str:
        return os.path.join(self.dir, self.template.format(self.indices[i]))

    @property
    def frame_size(self) -> Tuple[int, int]:
        """(H, W) of the video: that of its first frame"""
        if self._size is None:
            from PIL import Image
            with Image.open(self.path(0)) as im:
                self._size = (im.size[1], im.size[0])
        return self._size

    def pool(self) -> ThreadPoolExecutor:
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=self.threads)
        return self._pool

    def borrow(self, pool: ThreadPoolExecutor, side=None) -> None:
        """decode on `pool`, which stays its owner's: `close()` leaves it running (encode_videos lends one pool to every reader
        of a run).  `side`: the owner's copy stream, for the readers that put work on one"""
        self.close()
        self._pool, self._borrowed = pool, True

    def close(self):
        if self._pool is not None and not self._borrowed:
            self._pool.shutdown(wait=True)
        self._pool, self._borrowed = None, False

    def _decode(self, i: int, dst: np.ndarray):
        from PIL import Image
        p = self.path(i)
        with Image.open(p) as im:
            a = np.asarray(im.convert("RGB"))
        if a.shape != dst.shape:
            raise ValueError(f"{p}: frame is {a.shape[0]} x {a.shape[1]}, the video's first frame is {dst.shape[0]} x {dst.shape[1]}")
        dst[...] = a

    def _fill(self, i0: int, i1: int, slot: int) -> torch.Tensor:
        H, W = self.frame_size
        if self.copied[slot] is not None:             # the copy that read this buffer two batches ago must be over
            self.copied[slot].synchronize()
            self.copied[slot] = None
        buf = self._buf[slot]
        if buf is None or buf.shape[0] < i1 - i0:
            buf = torch.empty(i1 - i0, H, W, 3, dtype=torch.uint8)
            buf = buf.pin_memory() if self.pinned else buf
            self._buf[slot] = buf
        view = buf[: i1 - i0]
        dst = view.numpy()
        list(self.pool().map(lambda j: self._decode(i0 + j, dst[j]), range(i1 - i0)))
        return view

    def decode_batch(self, i0: int, i1: int, slot: int) -> torch.Tensor:
        """the host stage of one batch, on its own (measurements): frames i0 ... i1 - 1 decoded into the slot's buffer"""
        return self._fill(i0, i1, slot)

    def decode_into(self, i0: int, i1: int, dst: np.ndarray) -> list:
        """frames i0 ... i1 - 1 into the caller's uint8 [i1 - i0, H, W, 3] `dst`, on the pool: the futures, one per frame, so that
        the caller can have several videos' frames decoded at once and wait for all of them"""
        assert dst.shape == (i1 - i0, *self.frame_size, 3) and dst.dtype == np.uint8, (dst.shape, dst.dtype)
        pool = self.pool()
        return [pool.submit(self._decode, i0 + j, dst[j]) for j in range(i1 - i0)]

    def batches(self, n: int) -> Iterator[Tuple[int, torch.Tensor]]:
        """(slot, uint8 [k, H, W, 3]) for consecutive groups of n frames; batch k + 1 is being decoded while k is consumed.  The
        consumer of an asynchronous copy stores its event in `self.copied[slot]`: the slot is refilled only after it."""
        T = len(self)
        spans = [(i, min(T, i + n)) for i in range(0, T, n)]
        with ThreadPoolExecutor(max_workers=1) as driver:
            try:
                fut = driver.submit(self._fill, *spans[0], 0)
                for k in range(len(spans)):
                    view = fut.result()
                    fut = driver.submit(self._fill, *spans[k + 1], (k + 1) & 1) if k + 1 < len(spans) else None
                    yield k & 1, view
            finally:
                self.close()


class _ArrayFrames:
    """decoded frames already in memory ([T, H, W, 3] uint8, pinned or not): the same interface, nothing to decode"""

    def __init__(self, frames):
        self.frames = torch.as_tensor(frames)
        if self.frames.dtype != torch.uint8 or self.frames.dim() != 4 or self.frames.shape[-1] != 3:
            raise ValueError("frames must be uint8 [T, H, W, 3]")
        self.copied = [None, None]

    def __len__(self):
        return self.frames.shape[0]

    def batches(self, n: int):
        for k, i in enumerate(range(0, len(self), n)):
            yield k & 1, self.frames[i:i + n]


# ---------------------------------------------------------------------------------------------------------------- writer
def feature_path(out_path: str) -> str:
    return out_path if out_path.endswith(".npy") else out_path + ".npy"


def is_complete(out_path: str, shape: Tuple[int, int], dtype: str = "float32") -> bool:
    """an existing feature file whose header states `dtype` (float32, float16) and `shape`; a leftover `.tmp` beside it does not
    count, and neither does a file of the other dtype: asking for float16 where float32 files lie rewrites them, and back"""
    from .feature_stream import FeatureStream
    p = feature_path(out_path)
    if not os.path.isfile(p):
        return False
    try:
        with open(p, "rb") as fh:
            got, fortran, have = FeatureStream._npy_header(fh)
    except Exception:
        return False
    return tuple(got) == tuple(shape) and not fortran and have == np.dtype("<f2" if dtype == "float16" else "<f4")


def write_features(out_path: str, rows: np.ndarray) -> str:
    """np.save format, float32 [T * ncrops, D] (float16 rows stay float16): written beside its place as `<out>.npy.tmp` (a stale
    one is replaced), then moved into place atomically -- a reader never sees a half-written file under the final name"""
    p = feature_path(out_path)
    rows = np.ascontiguousarray(rows, dtype=np.float16 if np.asarray(rows).dtype == np.float16 else np.float32)
    assert rows.ndim == 2
    os.makedirs(os.path.dirname(os.path.abspath(p)), exist_ok=True)
    tmp = p + ".tmp"
    with open(tmp, "wb") as fh:
        np.save(fh, rows, allow_pickle=False)
    os.replace(tmp, p)
    return p


class FeatureWriter:
    """One thread that writes feature files behind the encode loop (`extract_dataset(pack=True)`).  `acquire()` takes one of
    `max_inflight` places for a video's row buffer and blocks while all are taken; `submit(event, rows, out_path)` hands the
    filled buffer over: the thread waits for `event` (anything with `synchronize()`, or None), calls `write_features` and gives
    the place back.  `overflow` (a pinned int64 [1] that the same event covers: float16 rows) is looked at before the write: non-zero
    is a ValueError naming the file, and nothing is written.  The first exception is kept: every job behind it is dropped unwritten (its place is still given back, so
    the producer never waits for a dead writer), the `.npy.tmp` of the failed write is removed, and `check()` / `close()`
    raise it in the caller's thread -- `close()` after the thread has been joined."""

    def __init__(self, max_inflight: int = 4, done=None):
        self.error = None
        self._done = done                              # called in the writer thread after each file: done(tag)
        self._places = threading.Semaphore(max(1, int(max_inflight)))
        self._jobs = queue.SimpleQueue()
        self._thread = threading.Thread(target=self._run, name="acx-feature-writer", daemon=True)
        self._thread.start()

    def acquire(self) -> None:
        self._places.acquire()
        self.check()

    def submit(self, event, rows, out_path: str, tag=None, overflow=None) -> None:
        self._jobs.put((event, rows, out_path, tag, overflow))

    def check(self) -> None:
        if self.error is not None:
            raise self.error

    def _run(self):
        while True:
            job = self._jobs.get()
            if job is None:
                return
            event, rows, out_path, tag, overflow = job
            try:
                if self.error is None:
                    if event is not None:
                        event.synchronize()
                    check_overflow(overflow, out_path)
                    write_features(out_path, rows.numpy() if isinstance(rows, torch.Tensor) else rows)
                    if self._done is not None:
                        self._done(tag)
            except BaseException as e:                  # (kept for the caller; the thread goes on giving places back)
                self.error = e
                try:
                    os.remove(feature_path(out_path) + ".tmp")
                except OSError:
                    pass
            finally:
                del job, rows
                self._places.release()

    def close(self, check: bool = True) -> None:
        """every job handed over so far is written (or dropped behind a failure), the thread is joined, then `check()`"""
        if self._thread is not None:
            self._jobs.put(None)
            self._thread.join()
            self._thread = None
        if check:
            self.check()


# ---------------------------------------------------------------------------------------------------------------- extractor
def _half_buffer(shape: Tuple[int, int]):
    """(rows, count): pinned float16 `shape` and, behind it in the same allocation, the int64 [1] that the overflow counter of the
    casts is copied into"""
    n = shape[0] * shape[1] * 2
    pad = -n % 8
    buf = torch.empty(n + pad + 8, dtype=torch.uint8).pin_memory()
    return buf[:n].view(torch.float16).view(shape), buf[n + pad:].view(torch.int64)


def check_overflow(count, out_path: str) -> None:
    """count: the (synchronised) overflow counter of a video's casts, or None"""
    n = 0 if count is None else int(count.reshape(-1)[0])
    if n:
        raise ValueError(f"{feature_path(out_path)}: {n} feature value(s) do not fit float16 (|x| >= 65520 rounds to infinity); "
                         f"not written: extract this video with dtype='float32'")


def _encoder_of(net_or_encoder):
    return getattr(net_or_encoder, "image_encoder", net_or_encoder)


def batch_frames(encoder, ncrops: int) -> int:
    """frames per batch: one encoder launch of at most `encoder.chunk` rows"""
    return max(1, int(encoder.chunk) // ncrops)


def check_eval_mode(encoder) -> None:
    if encoder.training and any(isinstance(m, torch.nn.modules.batchnorm._BatchNorm) for m in encoder.modules()):
        raise ValueError(f"{getattr(encoder, 'arch', type(encoder).__name__)}: extraction needs eval mode (call .eval()): in "
                         "training mode BatchNorm takes its statistics from each batch")


def check_encoder(encoder) -> None:
    """what the encode loop needs of the image encoder: eval mode where it has BatchNorm, and the GPU"""
    check_eval_mode(encoder)
    if next(encoder.parameters()).device.type != "cuda":
        raise ValueError("the encoder must be on the GPU")


def encode_video(encoder, frames, ncrops: int = 1, scale_size: Optional[int] = None) -> Iterator[Tuple[int, torch.Tensor]]:
    """The encode loop of one video (a FrameFolderReader, or decoded uint8 frames [T, H, W, 3]): yields (row0, rows) -- `rows`
    float32 [k * ncrops, D] on the device, queued on the current stream, the rows row0 ... of the video's [T * ncrops, D] table.
    `batch_frames(encoder, ncrops)` frames per encoder launch; the frames reach the device on a side stream.  The consumer copies
    each block where it wants it (a pinned file buffer: extract_video; a slice of a resident bank: FeatureBank.from_frames)."""
    from .preprocess import preprocess_crops
    encoder = _encoder_of(encoder)
    check_encoder(encoder)
    reader = frames if hasattr(frames, "batches") else _ArrayFrames(frames)
    R = int(encoder.input_resolution)
    dev = next(encoder.parameters()).device
    cur = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(device=dev)
    r0 = 0
    for slot, view in reader.batches(batch_frames(encoder, ncrops)):
        with torch.cuda.stream(side):
            x8 = view.to(dev, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
        reader.copied[slot] = ev
        cur.wait_event(ev)
        x8.record_stream(cur)
        with torch.no_grad():                     # (per batch: a grad mode held across a yield would reach the consumer)
            x = preprocess_crops(x8, R, scale_size, ncrops)
            rows = encoder(x.view(-1, 3, R, R))
        yield r0, rows
        r0 += rows.shape[0]
    assert r0 == len(reader) * ncrops, (r0, len(reader), ncrops)


def extract_video(encoder, frames, out_path: str, ncrops: int = 1, scale_size: Optional[int] = None, overwrite: bool = False,
                  decode: str = "pil", dtype: str = "float32") -> dict:
    """Encodes the frames of one video (a FrameFolderReader, or decoded uint8 frames [T, H, W, 3]) into `out_path` (.npy).
    decode="gpu" / "gpu_entropy": the frames of a FrameFolderReader are read by a jpeg.JpegFolderReader /
    jpeg.JpegEntropyFolderReader over the same files instead.
    dtype: "float32", or "float16" (rounded on the device, block by block; ValueError and no file if a value does not fit).
    Returns {"written": bool, "frames": T, "rows": T * ncrops}."""
    from . import jpeg, ops
    check_dtype(dtype)
    jpeg.check_decode(decode)
    encoder = _encoder_of(encoder)
    reader = frames if hasattr(frames, "batches") else _ArrayFrames(frames)
    if decode != "pil" and isinstance(reader, FrameFolderReader) and not isinstance(reader, jpeg.JpegFolderReader):
        reader = jpeg.READERS[decode].like(reader)
    T, D = len(reader), int(encoder.output_dim)
    shape = (T * ncrops, D)
    check_eval_mode(encoder)
    if not overwrite and is_complete(out_path, shape, dtype):
        return {"written": False, "frames": T, "rows": shape[0]}
    check_encoder(encoder)
    dev = next(encoder.parameters()).device
    if dtype == "float16":
        out, count = _half_buffer(shape)
        over = torch.zeros(1, dtype=torch.int64, device=dev)
    else:
        out, count, over = torch.empty(shape, dtype=torch.float32).pin_memory(), None, None
    for r0, rows in encode_video(encoder, reader, ncrops, scale_size):
        if over is not None:
            rows = ops.cast_rows_f16(rows, over)
        out[r0:r0 + rows.shape[0]].copy_(rows, non_blocking=True)
    if over is not None:
        count.copy_(over, non_blocking=True)          # read once, behind the last block, by the synchronisation below
    torch.cuda.current_stream(dev).synchronize()
    check_overflow(count, out_path)
    write_features(out_path, out.numpy())
    return {"written": True, "frames": T, "rows": shape[0]}


# ---------------------------------------------------------------------------------------------------------------- packed
SLOT_ALIGN = 256        # a group's first byte in a launch's frame buffer: the crop kernel reads whole 16-byte blocks from its base


def _iter_launches(lengths: Iterable[int], nb: int) -> Iterator[List[Tuple[int, int, int]]]:
    """plan_launches' launches, made as the lengths arrive: the next video's length is asked for only once the launch being
    filled has room for its first frame, so a full launch is out before the video behind it has to be opened"""
    launch, room = [], nb
    for v, T in enumerate(lengths):
        i = 0
        while i < T:
            k = min(room, T - i)
            launch.append((v, i, i + k))
            i, room = i + k, room - k
            if room == 0:
                yield launch
                launch, room = [], nb
    if launch:
        yield launch


def plan_launches(lengths: Sequence[int], ncrops: int, chunk: int) -> List[List[Tuple[int, int, int]]]:
    """The encoder launches of a packed run over videos of `lengths[v]` frames, in extraction order: each launch a list of pieces
    (v, i0, i1) -- frames i0 ... i1 - 1 of video v -- in video order, then frame order.  Every frame is in exactly one piece; a
    launch holds `max(1, chunk // ncrops)` frames (batch_frames), only the last one may hold fewer; a video without frames has no
    piece.  For one video these are encode_video's batches."""
    return list(_iter_launches([int(T) for T in lengths], max(1, int(chunk) // int(ncrops))))


class _Opener:
    """The run's readers, opened on the pool (listing a folder is host work like decoding) up to `lookahead` videos ahead of the
    one being decoded.  The iterable is advanced by one pool task at a time: it may be a generator."""

    def __init__(self, readers, pool: ThreadPoolExecutor, lookahead: int):
        self.it, self.pool, self.lookahead = iter(readers), pool, max(0, int(lookahead))
        self.ready, self.fut, self.exhausted = deque(), None, False

    def _open(self, n: int):
        got = []
        for _ in range(n):
            try:
                got.append(next(self.it))
            except StopIteration:
                return got, None, True
            except BaseException as e:                  # (what was opened before it is still handed over, then the error)
                return got, e, True
        return got, None, False

    def _collect(self):
        got, err, end = self.fut.result()
        self.fut = None
        self.ready.extend(got)
        self.exhausted |= end
        if err is not None:
            self.error = err

    error = None

    def top_up(self):
        if self.fut is not None and self.fut.done():
            self._collect()
        if self.fut is None and not self.exhausted and len(self.ready) < self.lookahead:
            self.fut = self.pool.submit(self._open, self.lookahead - len(self.ready))

    def next(self):
        """the next (key, reader), or None after the last"""
        while True:
            if self.ready:
                item = self.ready.popleft()
                self.top_up()
                return item
            if self.fut is not None:
                self._collect()
            elif self.error is not None:
                raise self.error
            elif self.exhausted:
                return None
            else:
                self.fut = self.pool.submit(self._open, max(1, self.lookahead))

    def close(self):
        if self.fut is not None:
            self._collect()
        for _, reader in self.ready:
            reader.close()
        self.ready.clear()


class _Piece:
    __slots__ = ("key", "reader", "i0", "i1", "off", "nbytes", "hw", "token")


class _Launch:
    __slots__ = ("slot", "host", "frames_dev", "pieces")


class _LaunchFeeder(threading.Thread):
    """The host side of encode_videos, one launch ahead of the encode: this thread opens the readers, cuts their frames into
    launches (_iter_launches) and has every piece of a launch decoded on the shared pool -- a FrameFolderReader's into the
    launch's slot of the pinned ring, a device reader's (jpeg.py) through its own pinned buffers into the launch's device frame
    buffer.  It starts on launch k + 1 when the consumer takes launch k, whichever videos the two belong to."""

    def __init__(self, readers, pool, lookahead: int, nb: int, dev, side):
        super().__init__(name="acx-launch-feeder", daemon=True)
        self.opener = _Opener(readers, pool, lookahead)
        self.pool, self.nb, self.dev, self.side = pool, nb, dev, side
        self.pinned = True
        self.ring = [None, None, None]                 # the pinned uint8 ring: three slots of one launch's frames
        self.copied = [None, None, None]               # per slot: the consumer's event after the copies that READ it
        self.frame_bytes = 0                           # the largest frame met so far
        self.active = []                               # v -> (key, reader), None once the video's last frame is decoded
        self._out = queue.SimpleQueue()
        self._credit = threading.Semaphore(1)
        self._halt = False

    # ------------------------------------------------------------------------------------------------------------ consumer
    def take(self) -> Optional[_Launch]:
        """the next decoded launch (None after the last; the feeder's exception is raised here), and leave to decode another"""
        item = self._out.get()
        if isinstance(item, BaseException):
            raise item
        self._credit.release()
        return item

    def stop(self):
        self._halt = True
        self._credit.release()
        if self.is_alive():
            self.join()
        self.opener.close()
        for kr in self.active:
            if kr is not None:
                kr[1].close()
        self.active = []

    # ------------------------------------------------------------------------------------------------------------ thread
    def _lengths(self):
        while True:
            kr = self.opener.next()
            if kr is None:
                return
            kr[1].borrow(self.pool, self.side)
            self.active.append(kr)
            yield len(kr[1])

    def _slot(self, k: int) -> Tuple[int, torch.Tensor]:
        s = k % 3
        if self.copied[s] is not None:                 # the copies that read this slot three launches ago must be over
            self.copied[s].synchronize()
            self.copied[s] = None
        need = self.nb * (-(-self.frame_bytes // SLOT_ALIGN) * SLOT_ALIGN + SLOT_ALIGN)
        if self.ring[s] is None or self.ring[s].numel() < need:
            buf = torch.empty(need, dtype=torch.uint8)
            self.ring[s] = buf.pin_memory() if self.pinned else buf
        return s, self.ring[s]

    def _decode(self, k: int, plan) -> _Launch:
        L = _Launch()
        L.pieces, off, prev = [], 0, None
        for v, i0, i1 in plan:
            p = _Piece()
            p.key, p.reader = self.active[v]
            p.i0, p.i1, p.hw, p.token = i0, i1, tuple(p.reader.frame_size), None
            kind = (p.hw, bool(getattr(p.reader, "device_frames", False)))
            if kind != prev or kind[1]:                # a new group: host pieces of one geometry side by side are one block of
                off = -(-off // SLOT_ALIGN) * SLOT_ALIGN    # frames; a device decoder's piece starts on a boundary of its own
                prev = kind
            p.off, p.nbytes = off, (i1 - i0) * p.hw[0] * p.hw[1] * 3
            off += p.nbytes
            self.frame_bytes = max(self.frame_bytes, p.hw[0] * p.hw[1] * 3)
            L.pieces.append(p)
        total = -(-off // SLOT_ALIGN) * SLOT_ALIGN
        with torch.cuda.stream(self.side):
            L.frames_dev = torch.empty(total, dtype=torch.uint8, device=self.dev)
        L.slot, L.host = None, None
        host = [p for p in L.pieces if not getattr(p.reader, "device_frames", False)]
        futs = []
        if host:
            L.slot, ring = self._slot(k)
            L.host = ring[:total]
            flat = L.host.numpy()
            for p in host:
                dst = flat[p.off:p.off + p.nbytes].reshape(p.i1 - p.i0, p.hw[0], p.hw[1], 3)
                futs += p.reader.decode_into(p.i0, p.i1, dst)
        for p in L.pieces:
            if p not in host:                          # (their frames are being decoded on the pool's other threads meanwhile)
                dst = L.frames_dev[p.off:p.off + p.nbytes].view(p.i1 - p.i0, p.hw[0], p.hw[1], 3)
                p.token = p.reader.decode_into(p.i0, p.i1, dst)
        err = None
        for f in futs:                                 # every frame is waited for: none is written after the launch is let go
            try:
                f.result()
            except BaseException as e:
                err = err or e
        if err is not None:
            raise err
        for v, i0, i1 in plan:
            if i1 == len(self.active[v][1]):
                self.active[v] = None                  # (the pieces hold the reader until the consumer is through with them)
        return L

    def run(self):
        try:
            torch.cuda.set_device(self.dev)
            plans = _iter_launches(self._lengths(), self.nb)
            k = 0
            while True:
                self._credit.acquire()                 # (before the launch is planned: planning may open a reader)
                if self._halt:
                    return
                plan = next(plans, None)
                if plan is None:
                    break
                self.opener.top_up()
                self._out.put(self._decode(k, plan))
                k += 1
            self._out.put(None)
        except BaseException as e:
            self._out.put(e)


def encode_videos(encoder, readers, ncrops: int = 1, scale_size: Optional[int] = None, lookahead: int = 2,
                  decode_threads: int = 8) -> Iterator[Tuple[object, int, torch.Tensor]]:
    """encode_video over many videos with the encoder kept full across their boundaries.  `readers`: an iterable of
    (key, reader), opened lazily (a generator: beside the readers of the launch being encoded and of the launch being decoded, at
    most `lookahead` are open ahead of them, and a reader is closed after its last frame).  Yields (key, row0, rows): `rows` float32 [k * ncrops, D] on the device, queued on the current
    stream, the rows row0 ... of video `key`'s [T * ncrops, D] table -- in video order, then row order.

    The launches are plan_launches': every one but the last holds batch_frames(encoder, ncrops) frames, of as many videos as it
    takes, and is ONE encoder call.  A launch's frames are decoded while the launch before it is encoded, by one pool of
    `decode_threads` threads (at most MAX_DECODE_THREADS) that also opens the readers, into one pinned uint8 ring of three
    slots that lasts the whole run (device readers: through their own pinned buffers).  Pieces of one frame size side by side
    are one group: one copy (or the device decoder's launches) into the launch's frame buffer and one preprocess_crops call into
    the group's slice of the launch's [rows, 3, R, R] input.  Ordering is by events only: nothing here synchronises the device."""
    from .preprocess import preprocess_crops
    encoder = _encoder_of(encoder)
    check_encoder(encoder)
    R = int(encoder.input_resolution)
    dev = next(encoder.parameters()).device
    cur = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(device=dev)
    pool = ThreadPoolExecutor(max_workers=max(1, min(int(decode_threads), MAX_DECODE_THREADS)), thread_name_prefix="acx-decode")
    feeder = _LaunchFeeder(readers, pool, lookahead, batch_frames(encoder, ncrops), dev, side)
    try:
        feeder.start()
        while True:
            L = feeder.take()
            if L is None:
                break
            groups = []                                # [off, frames, (H, W)]: runs of pieces in one block of the frame buffer
            for p in L.pieces:
                if groups and groups[-1][0] + groups[-1][1] * groups[-1][2][0] * groups[-1][2][1] * 3 == p.off and groups[-1][2] == p.hw:
                    groups[-1][1] += p.i1 - p.i0
                else:
                    groups.append([p.off, p.i1 - p.i0, p.hw])
            if L.host is not None:
                with torch.cuda.stream(side):
                    for p in L.pieces:
                        if p.token is None:
                            L.frames_dev[p.off:p.off + p.nbytes].copy_(L.host[p.off:p.off + p.nbytes], non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(side)
                feeder.copied[L.slot] = ev
                cur.wait_event(ev)
            for p in L.pieces:
                if p.token is not None:
                    p.reader.finish_into(p.token)      # (makes the current stream wait for the piece's frames)
            L.frames_dev.record_stream(cur)
            nrows = sum(g[1] for g in groups) * ncrops
            with torch.no_grad():                      # (per launch: a grad mode held across a yield would reach the consumer)
                x = torch.empty(nrows, 3, R, R, dtype=torch.float32, device=dev)
                r = 0
                for off, n, (H, W) in groups:
                    preprocess_crops(L.frames_dev[off:off + n * H * W * 3].view(n, H, W, 3), R, scale_size, ncrops,
                                     out=x[r:r + n * ncrops])
                    r += n * ncrops
                rows = encoder(x)
            assert rows.shape[0] == nrows, (rows.shape, nrows)
            r = 0
            for p in L.pieces:
                n = (p.i1 - p.i0) * ncrops
                yield p.key, p.i0 * ncrops, rows[r:r + n]
                r += n
                if p.i1 == len(p.reader):
                    p.reader.close()
    finally:
        feeder.stop()
        pool.shutdown(wait=True)


class _InOrder:
    """log lines that arrive in any order, from any thread, given to `log` in video order"""

    def __init__(self, log):
        self.log, self.pending, self.next, self.lock = log, {}, 0, threading.Lock()

    def put(self, idx: int, line: str):
        with self.lock:
            self.pending[idx] = line
            while self.next in self.pending:
                line = self.pending.pop(self.next)
                self.next += 1
                if self.log:
                    self.log(line)


def _extract_dataset_packed(encoder, videos, frames_root, out_root, ncrops, scale_size, overwrite, template, decode_threads, log,
                            decode, max_inflight, dtype="float32") -> dict:
    """extract_dataset(pack=True): encode_videos over the videos whose files are not complete; each video's rows are copied into a
    pinned buffer of its own, at most `max_inflight` of them alive, and written by a FeatureWriter behind the encode loop"""
    from . import jpeg, ops
    check_eval_mode(encoder)
    D = int(encoder.output_dim)
    todo, results, lines = {}, {}, _InOrder(log)
    half = dtype == "float16"

    def line(idx, video):
        written, _, rows = results[idx]
        return f"{'wrote' if written else 'kept '} {feature_path(os.path.join(out_root, video))}  [{rows} rows]"

    def readers():
        for idx, (video, start, end) in enumerate(videos):
            reader = jpeg.make_reader(decode, frames_root, video, start, end, template, decode_threads)
            T, out_path = len(reader), os.path.join(out_root, video)
            if not overwrite and is_complete(out_path, (T * ncrops, D), dtype):
                reader.close()
                results[idx] = (False, T, T * ncrops)
                lines.put(idx, line(idx, video))
                continue
            todo[idx] = (video, out_path, T)
            yield idx, reader

    def written(idx):
        video, _, T = todo[idx]
        results[idx] = (True, T, T * ncrops)
        lines.put(idx, line(idx, video))

    writer = FeatureWriter(max_inflight, done=written)
    gen = encode_videos(encoder, readers(), ncrops, scale_size, decode_threads=decode_threads)
    cur_idx, out, count, over = None, None, None, None
    try:
        for idx, r0, rows in gen:
            _, out_path, T = todo[idx]
            if idx != cur_idx:
                writer.acquire()                       # (blocks while max_inflight videos' buffers are alive)
                cur_idx = idx
                if half:                               # the video's own overflow counter: its casts add to it, the writer reads it
                    out, count = _half_buffer((T * ncrops, D))
                    over = torch.zeros(1, dtype=torch.int64, device=rows.device)
                else:
                    out = torch.empty((T * ncrops, D), dtype=torch.float32).pin_memory()
            if half:
                rows = ops.cast_rows_f16(rows, over)
            out[r0:r0 + rows.shape[0]].copy_(rows, non_blocking=True)
            if r0 + rows.shape[0] == T * ncrops:
                if half:
                    count.copy_(over, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(rows.device))
                writer.submit(ev, out, out_path, idx, count)
                out, count, over = None, None, None
    finally:
        gen.close()
        writer.close(check=False)
    writer.check()
    counts = {"written": 0, "skipped": 0, "frames": 0, "rows": 0}
    for idx in sorted(results):
        w, T, rows = results[idx]
        counts["written" if w else "skipped"] += 1
        if w:
            counts["frames"] += T
            counts["rows"] += rows
    return counts


def list_videos(frames_root: str, template: str = TEMPLATE) -> List[str]:
    """every folder under frames_root that holds a file matching the template, relative to it, sorted"""
    rx = _template_regex(template)
    out = []
    for d, subdirs, files in os.walk(frames_root):
        subdirs.sort()
        if any(rx.fullmatch(f) for f in files):
            out.append(os.path.relpath(d, frames_root))
    return sorted(out)


def extract_dataset(net_or_encoder, annotation_file: Optional[str], frames_root: str, out_root: str, ncrops: int = 1,
                    scale_size: Optional[int] = None, overwrite: bool = False, template: str = TEMPLATE,
                    decode_threads: int = 8, log=None, decode: str = "pil", pack: bool = False, max_inflight: int = 4,
                    dtype: str = "float32") -> dict:
    """Every video of the annotation file (rows `path start end label...`; without one: every frame folder under frames_root)
    -> `<out_root>/<path>.npy`.  Complete files are skipped unless overwrite.  decode: "pil" (Pillow on the host), "gpu" (baseline
    JPEG reconstructed on the device; every other file through Pillow) or "gpu_entropy" (its Huffman decoding on the device too).
    pack: the videos share encoder launches (encode_videos: every launch but the last is full, and the next video is decoded
    while this one is encoded) and the files are written by a thread behind the encode loop, at most `max_inflight` videos'
    rows waiting for it; the same files to round-off, the same counts and log lines.
    dtype: "float32" or "float16" files (extract_video); a present file of the other dtype is rewritten, not kept.
    Returns {written, skipped, frames, rows}."""
    from . import jpeg
    check_dtype(dtype)
    jpeg.check_decode(decode)
    encoder = _encoder_of(net_or_encoder)
    if annotation_file:
        videos = read_annotations(annotation_file)
    else:
        videos = [(v, None, None) for v in list_videos(frames_root, template)]
    if pack:
        return _extract_dataset_packed(encoder, videos, frames_root, out_root, ncrops, scale_size, overwrite, template,
                                       decode_threads, log, decode, max_inflight, dtype)
    counts = {"written": 0, "skipped": 0, "frames": 0, "rows": 0}
    for video, start, end in videos:
        reader = jpeg.make_reader(decode, frames_root, video, start, end, template, decode_threads)
        try:
            r = extract_video(encoder, reader, os.path.join(out_root, video), ncrops, scale_size, overwrite, dtype=dtype)
        finally:
            reader.close()
        counts["written" if r["written"] else "skipped"] += 1
        if r["written"]:
            counts["frames"] += r["frames"]
            counts["rows"] += r["rows"]
        if log:
            log(f"{'wrote' if r['written'] else 'kept '} {feature_path(os.path.join(out_root, video))}  [{r['rows']} rows]")
    return counts


# ---------------------------------------------------------------------------------------------------------------- command line
def build_image_encoder(arch: str, precision: str = "auto", chunk: int = 512, act: Optional[str] = None):
    """the CLIP image encoder of `arch`, as AnomalyCLIP builds it.  act: the ViT MLP's activation, "quick_gelu" (OpenAI's weights) or
    "gelu" (open_clip's LAION-2B / DataComp weights), None: the arch's own ("gelu" for ViT-H-14, "quick_gelu" otherwise); "gelu" with
    precision "bf16" or a ResNet arch is a ValueError naming both"""
    from .components.anomaly_clip import geometry_of_arch
    from .components.clip_resnet import ModifiedResNet
    from .components.clip_vit import VisionTransformer, check_act
    geom = geometry_of_arch(arch)
    act = act or geom.act
    check_act(act, precision, arch if geom.is_resnet else None)
    if geom.is_resnet:
        return ModifiedResNet(geom.vision_layers, geom.embed_dim, geom.resnet_heads, geom.image_resolution, geom.vision_width,
                              precision=precision, chunk=chunk, arch=arch)
    return VisionTransformer(geom.image_resolution, geom.vision_patch_size, geom.vision_width, geom.vision_layers,
                             geom.vision_heads, geom.embed_dim, precision=precision, chunk=chunk, arch=arch, act=act)


def load_encoder_weights(encoder, arch: str, weights) -> None:
    """weights: a Lightning .ckpt (`net.image_encoder.*`), a dict holding `state_dict`, an AnomalyCLIP state_dict
    (`image_encoder.*`), the encoder's own state_dict, or a plain CLIP state_dict (`visual.*`: OpenAI's model.state_dict(),
    open_clip's open_clip_pytorch_model.bin); a checkpoint of another backbone is a ValueError naming both."""
    from .checkpoint import from_clip_state_dict, is_clip_state_dict, split_lightning_state_dict
    from .components.anomaly_clip import _describe, geometry_from_state_dict, geometry_of_arch
    ck = torch.load(weights, map_location="cpu", weights_only=False) if isinstance(weights, str) else weights
    sd = ck.get("state_dict", ck) if isinstance(ck, dict) else ck
    sd = from_clip_state_dict(sd) if is_clip_state_dict(sd) else split_lightning_state_dict(sd)
    if not any(k.startswith("image_encoder.") for k in sd):
        sd = {"image_encoder." + k: v for k, v in sd.items()}
    theirs, mine = geometry_from_state_dict(sd), geometry_of_arch(arch)
    vision = ("image_resolution", "vision_layers", "vision_width", "vision_patch_size", "embed_dim")
    if theirs is not None and any(getattr(theirs, f) != getattr(mine, f) for f in vision):
        raise ValueError(f"the weights do not match arch {arch!r}: they hold {_describe(theirs)}, {arch} is {_describe(mine)}")
    encoder.load_state_dict({k[len("image_encoder."):]: v for k, v in sd.items() if k.startswith("image_encoder.")}, strict=True)


def _parser():
    import argparse
    from .components.anomaly_clip import _ARCH
    from .components.clip_resnet import RESNET_PRECISIONS
    from .components.clip_vit import PRECISIONS
    p = argparse.ArgumentParser(prog="python -m anomalyclip_amd.extract", description="CLIP feature files from frame folders")
    p.add_argument("--arch", required=True, choices=sorted(_ARCH))
    p.add_argument("--weights", required=True, help="Lightning .ckpt, AnomalyCLIP state_dict, image-encoder state_dict or plain CLIP state_dict")
    class _Act(argparse.Action):                         # (the parser's default stays "quick_gelu"; parse_args reads whether it was given)
        def __call__(self, parser, namespace, values, option_string=None):
            namespace.act, namespace.act_given = values, True
    p.set_defaults(act_given=False)
    p.add_argument("--act", default="quick_gelu", choices=("quick_gelu", "gelu"), action=_Act,
                   help="the ViT MLP's activation: quick_gelu for OpenAI's weights, gelu for open_clip weights trained without quick_gelu "
                        "(LAION-2B, DataComp); the weights do not say which.  Left out with --arch ViT-H-14 (open_clip weights only): gelu")
    p.add_argument("--frames-root", required=True)
    p.add_argument("--out-root", required=True)
    p.add_argument("--annotations", default=None, help="rows `path start end label...`; default: every folder of --frames-root")
    p.add_argument("--ncrops", type=int, default=1, choices=(1, 5, 10))
    p.add_argument("--scale-size", type=int, default=None, help="shorter side before cropping (default: crop, or crop * 8 // 7)")
    p.add_argument("--precision", default="auto", choices=sorted(set(PRECISIONS) | set(RESNET_PRECISIONS)))
    p.add_argument("--overwrite", action="store_true")
    p.add_argument("--decode", default="pil", choices=("pil", "gpu", "gpu_entropy"),
                   help="pil: Pillow on the host; gpu: baseline JPEG, Huffman decoding on the host and the rest on the device; "
                        "gpu_entropy: the Huffman decoding on the device too")
    p.add_argument("--dtype", default="float32", choices=DTYPES,
                   help="element type of the files: float16 halves them (rounded to nearest even on the device; a value that does "
                        "not fit is an error)")
    p.add_argument("--pack", action="store_true",
                   help="share encoder launches between videos and write the files behind the encode loop (many short clips)")
    return p


def parse_args(argv: Optional[Sequence[str]] = None):
    """argparse's behaviour for unknown arguments (exit status 2, `unrecognized arguments: ...`), and the same exit for arguments
    that contradict each other: a --scale-size below the arch's resolution, a --precision the arch's encoder does not run."""
    from .components.anomaly_clip import geometry_of_arch
    from .components.clip_resnet import check_resnet_precision
    from .components.clip_vit import check_act, check_vit_precision
    p = _parser()
    a = p.parse_args(argv)
    geom = geometry_of_arch(a.arch)
    if a.scale_size is not None and a.scale_size < geom.image_resolution:
        p.error(f"--scale-size {a.scale_size} conflicts with --arch {a.arch}: its crops are {geom.image_resolution} pixels")
    try:
        if geom.is_resnet:
            check_resnet_precision(a.precision, a.arch, geom.vision_width)
        else:
            check_vit_precision(a.precision, geom.grid ** 2 + 1, geom.vision_width, a.arch, geom.image_resolution, geom.vision_patch_size,
                                geom.vision_head_dim)
    except ValueError as e:
        p.error(f"--precision {a.precision} conflicts with --arch {a.arch}: {e}")
    if not a.act_given:
        a.act = geom.act                                   # the arch's own: "gelu" for ViT-H-14, the parser's default otherwise
    try:
        check_act(a.act, a.precision, a.arch if geom.is_resnet else None, key="--act")
    except ValueError as e:
        p.error(f"--act {a.act} conflicts with --precision {a.precision} / --arch {a.arch}: {e}")
    for name, path in (("--weights", a.weights), ("--frames-root", a.frames_root), ("--annotations", a.annotations)):
        if path is not None and not os.path.exists(path):
            p.error(f"{name} {path}: no such file or directory")
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    enc = build_image_encoder(a.arch, a.precision, act=a.act)
    load_encoder_weights(enc, a.arch, a.weights)
    enc = enc.to(torch.device("cuda", torch.cuda.current_device())).eval()
    counts = extract_dataset(enc, a.annotations, a.frames_root, a.out_root, a.ncrops, a.scale_size, a.overwrite,
                             log=lambda s: print(s, file=sys.stderr), decode=a.decode, pack=a.pack, dtype=a.dtype)
    import json
    print(json.dumps(counts))
    return 0


if __name__ == "__main__":
    sys.exit(main())
