"""Training batches from feature files: the whole training set resident in HBM, each batch drawn by ONE gather launch.

The reference's train-mode dataset (feature_dataset.py:260-276, :347-380) indexes N*L rows per video one Python tensor at a
time and the DataLoader then ships batch * N*L * D floats over PCIe for a step that takes ~11 ms on the device.  A feature set
fits in device memory (UCF-Crime: 1,610 training videos, ~25 GB), so here every `.npy` file is loaded once (`FeatureBank`)
and a step moves a few hundred bytes of indices: the video ids and the segment starts, drawn on the host in the reference's
order (`ResidentTrainLoader`: torch's sampler for the video order, one `randint` call per video for the starts), then
`acx_sample_segments` copies the rows (ops.sample_segments).

`FeatureBank.from_frames` fills the same bank from frame folders through the CLIP image encoder (no feature files), and
`BankTile` / `ops.tile_videos` draw the test-mode tiles out of a bank on the device."""
from __future__ import annotations

import os
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import feature_index as FI
from . import ops, parallel
from .feature_stream import FeatureStream

_STAGE_BYTES = 64 << 20          # pinned staging slot of the bank load (grown to the largest file)
BANK_DTYPES = {"float32": torch.float32, "float16": torch.float16}


def check_bank_dtype(bank_dtype) -> torch.dtype:
    """bank_dtype= of FeatureBank.from_frames / AnomalyCLIPDataModule: "float32" or "float16" """
    if bank_dtype not in BANK_DTYPES:
        raise ValueError(f"bank_dtype={bank_dtype!r}: a feature bank is 'float32' or 'float16'")
    return BANK_DTYPES[bank_dtype]


class FeatureBank:
    """Every feature file of `paths` in one device tensor `bank` [sum_v rows_v, D], files in order and rows as stored
    (frame t, crop c in row t * ncrops + c), in the files' element type `dtype`: float32, or float16 when every file is a
    half-precision one (the gathers widen the rows on their way out: every loader still yields float32).  `row_off` int64 [V], `frames` int32 [V] (rows_v // ncrops: what a frame index wraps
    around) and `labels` int64 [V] live on the device; `paths`, `num_frames` (the annotation rows' end - start + 1: what the
    train-mode draw is sized by), `file_frames`, `offsets` and `labels_host` on the host.  Under data parallelism every rank
    holds the full bank."""

    def __init__(self, paths: Sequence[str], num_frames: Sequence[int], labels: Sequence[int], ncrops: int = 1,
                 device: Optional[torch.device] = None, max_bytes: Optional[int] = None, readers: int = 4):
        self.paths = [str(p) for p in paths]
        self.num_frames = [int(n) for n in num_frames]
        self.labels_host = np.asarray([int(v) for v in labels], dtype=np.int64)
        self.ncrops = int(ncrops)
        if not (len(self.paths) == len(self.num_frames) == len(self.labels_host)):
            raise ValueError("FeatureBank: paths, num_frames and labels must have one entry per video")
        if self.ncrops <= 0:
            raise ValueError(f"FeatureBank: ncrops = {ncrops}")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        rows, self.D, dtype = self._scan()
        self.file_frames = [r // self.ncrops for r in rows]
        self.offsets = np.concatenate([[0], np.cumsum(rows, dtype=np.int64)]).astype(np.int64)       # [V + 1] bank rows
        need = int(self.offsets[-1]) * self.D * dtype.itemsize
        if max_bytes is None:
            with torch.cuda.device(self.device):
                max_bytes = int(torch.cuda.mem_get_info()[0] * 0.8)       # 80 % of what is free now: room left for the training step
        if need > max_bytes:
            raise ValueError(f"FeatureBank: {len(self.paths)} feature files need {need} bytes of device memory, "
                             f"{int(max_bytes)} bytes are available (banks larger than device memory are not supported)")
        self.bank = torch.empty(int(self.offsets[-1]), self.D, dtype=dtype, device=self.device)
        self._load(rows, max(1, int(readers)))
        self.row_off = torch.from_numpy(self.offsets[:-1].copy()).to(self.device)
        self.frames = torch.tensor(self.file_frames, dtype=torch.int32).to(self.device)
        self.labels = torch.from_numpy(self.labels_host).to(self.device)

    @classmethod
    def from_frames(cls, encoder, records, frames_root: str, image_tmpl: str = "{:06d}.jpg", ncrops: int = 1,
                    scale_size: Optional[int] = None, decode_threads: int = 8, device: Optional[torch.device] = None,
                    max_bytes: Optional[int] = None, log=None, decode: str = "pil", pack: bool = False,
                    bank_dtype: str = "float32") -> "FeatureBank":
        """The same bank, filled by the CLIP image encoder instead of from files: every frame an annotation row names
        (`records`: objects with `video`, `start_frame`, `end_frame`, `label`; frame t of video v is
        `<frames_root>/<video>/image_tmpl.format(t + start_frame)`, end inclusive) is decoded and encoded ONCE through
        extract.encode_video -- the launches `extract_video` makes, so the rows are the rows of the file it would write -- and each
        block of rows is copied from the encoder's output straight into its bank slice.  `paths` are the frame folders,
        `file_frames == num_frames`.  The size follows from the rows and `encoder.output_dim` and is checked before any frame is
        opened.  decode: "pil", "gpu" or "gpu_entropy", as extract.extract_dataset takes it.  pack: the videos share encoder
        launches (extract.encode_videos), each piece of rows copied into its video's bank slice: the same bank to round-off.
        bank_dtype: "float16" keeps the rows as halves -- each block is rounded on the device (ops.cast_rows_f16: to nearest even,
        as numpy rounds) on its way into the bank, half the memory; a feature too large for a half (|x| >= 65520) is a ValueError
        naming the video once the bank is filled."""
        from . import extract as X
        from . import jpeg
        jpeg.check_decode(decode)
        dtype = check_bank_dtype(bank_dtype)
        encoder = X._encoder_of(encoder)
        records = list(records)
        self = cls.__new__(cls)
        self.paths = [os.path.join(str(frames_root), r.video) for r in records]
        self.num_frames = [int(r.end_frame) - int(r.start_frame) + 1 for r in records]
        self.labels_host = np.asarray([int(r.label) for r in records], dtype=np.int64)
        self.ncrops, self.D = int(ncrops), int(encoder.output_dim)
        if self.ncrops not in (1, 5, 10):
            raise ValueError(f"FeatureBank.from_frames: ncrops = {ncrops} (1, 5 or 10 crops, as anomalyclip_amd.extract takes them)")
        if not records:
            raise ValueError("FeatureBank.from_frames: no videos")
        for p, n in zip(self.paths, self.num_frames):
            if n <= 0:
                raise ValueError(f"{p}: the annotation row holds {n} frames")
        if self.D % 4:
            raise ValueError(f"FeatureBank.from_frames: feature width {self.D} is not a multiple of 4")
        self.file_frames = list(self.num_frames)
        rows = [n * self.ncrops for n in self.num_frames]
        self.offsets = np.concatenate([[0], np.cumsum(rows, dtype=np.int64)]).astype(np.int64)
        need = int(self.offsets[-1]) * self.D * dtype.itemsize
        if max_bytes is None:
            with torch.cuda.device(next(encoder.parameters()).device):
                max_bytes = int(torch.cuda.mem_get_info()[0] * 0.8)       # 80 % of what is free now, as for a bank of files
        if need > max_bytes:
            raise ValueError(f"FeatureBank: the {int(self.offsets[-1]) // self.ncrops} frames of {len(records)} videos need {need} "
                             f"bytes of device memory at {self.ncrops} crop(s) x {self.D} {bank_dtype} values, {int(max_bytes)} bytes are "
                             f"available (banks larger than device memory are not supported; anomalyclip_amd.extract writes "
                             f"the same rows to feature files instead)")
        X.check_encoder(encoder)
        self.device = next(encoder.parameters()).device          # the rows never leave the device they are computed on
        if device is not None and (torch.device(device).type != "cuda" or torch.device(device).index not in (None, self.device.index)):
            raise ValueError(f"FeatureBank.from_frames: the encoder is on {self.device}, the bank was asked for on {device}")
        self.bank = torch.empty(int(self.offsets[-1]), self.D, dtype=dtype, device=self.device)
        # float16: one overflow counter per video, added to by the casts and read once, after the synchronisation below
        self._overflow = torch.zeros(len(records), dtype=torch.int64, device=self.device) if dtype == torch.float16 else None
        with torch.cuda.device(self.device):
            if pack:
                self._fill_packed(encoder, records, str(frames_root), image_tmpl, scale_size, decode_threads, decode, log, rows)
            for v, r in enumerate(() if pack else records):
                reader = jpeg.make_reader(decode, str(frames_root), r.video, int(r.start_frame), int(r.end_frame), image_tmpl,
                                          decode_threads)
                try:
                    self.fill_video(encoder, v, reader, scale_size)
                except FileNotFoundError as e:
                    raise FileNotFoundError(f"video {r.video!r}: frame file {e.filename} is missing (the annotation row names frames "
                                            f"{int(r.start_frame)} ... {int(r.end_frame)})") from e
                finally:
                    reader.close()
                if log:
                    log(f"encoded {self.paths[v]}  [{rows[v]} rows]")
            torch.cuda.current_stream().synchronize()           # the readers' pinned buffers are released on return
        self.check_overflow()
        self.row_off = torch.from_numpy(self.offsets[:-1].copy()).to(self.device)
        self.frames = torch.tensor(self.file_frames, dtype=torch.int32).to(self.device)
        self.labels = torch.from_numpy(self.labels_host).to(self.device)
        return self

    def _fill_packed(self, encoder, records, frames_root, image_tmpl, scale_size, decode_threads, decode, log, rows) -> None:
        """from_frames(pack=True): one extract.encode_videos run over every video; the bank's slices take the rows"""
        from . import extract as X
        from . import jpeg

        def readers():
            for v, r in enumerate(records):
                yield v, jpeg.make_reader(decode, frames_root, r.video, int(r.start_frame), int(r.end_frame), image_tmpl,
                                          decode_threads)

        gen = X.encode_videos(encoder, readers(), self.ncrops, scale_size, decode_threads=decode_threads)
        try:
            for v, r0, blk in gen:
                self._put(v, r0, blk)
                if log and r0 + blk.shape[0] == rows[v]:
                    log(f"encoded {self.paths[v]}  [{rows[v]} rows]")
        except FileNotFoundError as e:
            raise FileNotFoundError(f"frame file {e.filename} is missing (the annotation rows name every frame start ... end "
                                    f"of their videos)") from e
        finally:
            gen.close()

    def fill_video(self, encoder, v: int, frames, scale_size: Optional[int] = None) -> None:
        """encodes the frames of video v (a FrameFolderReader, or decoded uint8 frames [T, H, W, 3]) into its bank rows: every
        block of extract.encode_video is copied device to device into its slice, on the current stream"""
        from . import extract as X
        dst = self.video(v)
        if len(frames) * self.ncrops != dst.shape[0]:
            raise ValueError(f"{self.paths[v]}: {len(frames)} frames for {dst.shape[0] // self.ncrops} in the bank")
        for r0, blk in X.encode_video(encoder, frames, self.ncrops, scale_size):
            self._put(v, r0, blk)

    def _put(self, v: int, r0: int, blk: torch.Tensor) -> None:
        """a block of encoder rows into rows r0 ... of video v: a device-to-device copy, or the cast of a float16 bank"""
        dst = self.video(v)[r0:r0 + blk.shape[0]]
        if dst.dtype == torch.float16:
            if getattr(self, "_overflow", None) is None:
                self._overflow = torch.zeros(len(self.paths), dtype=torch.int64, device=self.device)
            ops.cast_rows_f16(blk, self._overflow[v:v + 1], out=dst)
        else:
            dst.copy_(blk)

    def check_overflow(self) -> None:
        """float16 bank filled from frames: raises ValueError for the first video with a feature that no half holds (the casts
        counted them on the device; call after the stream that ran them is synchronised).  from_frames does; after fill_video
        calls of one's own it is the caller's to call."""
        over = getattr(self, "_overflow", None)
        if over is None:
            return
        n = over.cpu().numpy()
        bad = np.flatnonzero(n)
        if bad.size:
            v = int(bad[0])
            raise ValueError(f"{self.paths[v]}: {int(n[v])} feature value(s) do not fit float16 (|x| >= 65520 rounds to infinity); "
                             f"{bad.size} video(s) affected: use bank_dtype='float32'")

    def __len__(self) -> int:
        return len(self.paths)

    @property
    def dtype(self) -> torch.dtype:
        """the bank's element type: torch.float32, or torch.float16 (half-precision feature files, bank_dtype="float16")"""
        return self.bank.dtype

    @property
    def nbytes(self) -> int:
        return self.bank.numel() * self.bank.element_size()

    def video(self, v: int) -> torch.Tensor:
        """the rows of video v as stored in its file: a view of the bank"""
        return self.bank[int(self.offsets[v]): int(self.offsets[v + 1])]

    def _scan(self) -> Tuple[List[int], int, torch.dtype]:
        rows, D, first = [], None, None
        for p in self.paths:
            with open(p, "rb") as fh:
                shape, fortran, dtype = FeatureStream._npy_header(fh)
            if len(shape) != 2 or fortran or dtype not in (np.dtype("<f4"), np.dtype("<f2")):
                raise ValueError(f"{p}: feature files must be C-ordered float32 (or float16) with two dimensions "
                                 f"(shape {tuple(shape)}, fortran_order {fortran}, dtype {dtype})")
            if first is None:
                first = (dtype, p)
            if dtype != first[0]:
                raise ValueError(f"{p}: dtype {dtype}, but {first[1]} and every file before this one hold {first[0]} (a bank has "
                                 f"one element type: float32 files or float16 files, not both)")
            if shape[0] == 0 or shape[0] % self.ncrops:
                raise ValueError(f"{p}: {shape[0]} rows are not a positive multiple of ncrops = {self.ncrops}")
            if D is None:
                D = int(shape[1])
            if shape[1] != D or D % 4:
                raise ValueError(f"{p}: feature width {shape[1]} (every file must have the same width, a multiple of 4; first file: {D})")
            rows.append(int(shape[0]))
        if D is None:
            raise ValueError("FeatureBank: no feature files")
        return rows, D, (torch.float16 if first[0] == np.dtype("<f2") else torch.float32)

    def _load(self, rows: List[int], readers: int) -> None:
        """files -> two pinned staging slots (filled by `readers` threads: file reads release the GIL) -> asynchronous copies into
        the bank; the files of a group are consecutive, so a group is ONE contiguous copy and the next group is read meanwhile."""
        from concurrent.futures import ThreadPoolExecutor
        D, esize = self.D, self.bank.element_size()              # (the slots hold the files' elements: halves stage half the bytes)
        slot_elems = max(_STAGE_BYTES // esize, max(rows) * D)
        groups, cur, used = [], [], 0
        for v, r in enumerate(rows):
            if cur and used + r * D > slot_elems:
                groups.append(cur)
                cur, used = [], 0
            cur.append(v)
            used += r * D
        groups.append(cur)
        slot_elems = min(slot_elems, max(sum(rows[v] for v in g) * D for g in groups))
        pinned = [torch.empty(slot_elems, dtype=self.bank.dtype).pin_memory() for _ in range(min(2, len(groups)))]
        copied: List[Optional[torch.cuda.Event]] = [None] * len(pinned)
        flat = self.bank.view(-1)

        def read(job):
            v, dst = job
            with open(self.paths[v], "rb") as fh:
                FeatureStream._npy_header(fh)
                got = fh.readinto(memoryview(dst).cast("B"))
            if got != dst.size * esize:
                raise IOError(f"{self.paths[v]}: short read ({got} of {dst.size * esize} bytes)")

        def fill(g, slot):
            if copied[slot] is not None:                      # the copy that last read this slot must be done before it is refilled
                copied[slot].synchronize()
            host, off, jobs = pinned[slot].numpy(), 0, []
            for v in g:
                n = rows[v] * D
                jobs.append((v, host[off:off + n]))
                off += n
            return jobs, off

        with ThreadPoolExecutor(max_workers=readers) as pool, torch.cuda.device(self.device):
            jobs, n = fill(groups[0], 0)
            pending = pool.map(read, jobs)
            for i, g in enumerate(groups):
                slot = i % len(pinned)
                list(pending)                                 # group i is in its slot (raises what a reader raised)
                n_i = n
                if i + 1 < len(groups):
                    jobs, n = fill(groups[i + 1], (i + 1) % len(pinned))
                    pending = pool.map(read, jobs)
                lo = int(self.offsets[g[0]]) * D
                flat[lo:lo + n_i].copy_(pinned[slot][:n_i], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                copied[slot] = ev
            torch.cuda.current_stream().synchronize()          # the pinned slots are released on return


class BankTile:
    """The test-mode tile of video `v` of a bank, not yet gathered: `[1, ncrops, rows, D]` with rows = N * L * S, row r = frame
    (r * stride) mod T (feature_index.test_start_indices).  `.to(device)` gathers it with one `acx_tile_videos` launch;
    AnomalyCLIPModule.score_videos gathers a whole group of them in one launch instead."""

    def __init__(self, bank: FeatureBank, v: int, num_segments: int, seg_length: int, stride: int = 1):
        self.bank, self.v = bank, int(v)
        self.N, self.L, self.stride = int(num_segments), int(seg_length), int(stride)
        starts, self.S = FI.test_start_indices(bank.file_frames[self.v], self.N, self.L, self.stride)
        self.rows = len(starts) * self.L
        self.shape = torch.Size((1, bank.ncrops, self.rows, bank.D))

    def dim(self) -> int:
        return 4

    def to(self, device=None, *unused, **unused_kw) -> torch.Tensor:
        b = self.bank
        if device is not None and torch.device(device).type != "cuda":
            raise ValueError("a BankTile is gathered on the bank's device")
        with torch.cuda.device(b.device):
            x = ops.tile_videos(b.bank, b.row_off, b.frames, [self.v], [self.S], self.N, self.L, self.stride, b.ncrops)
        return x.view(self.shape)

    def reshape(self, *shape) -> torch.Tensor:
        return self.to().reshape(*shape)


class _Indices(torch.utils.data.Dataset):
    """range(n) as a map-style dataset: what the samplers are built over"""

    def __init__(self, n: int):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return int(i)


class ResidentTrainLoader:
    """Iterable over the train-mode batches of `video_ids` (indices into `bank`): yields (features [b, ncrops, N*L, D] on the
    device, labels [b] int64 on the device) -- the tuples `AnomalyCLIPModule.model_step` unpacks.

    Video order: torch's RandomSampler / BatchSampler over range(len(video_ids)), driven by a DataLoader over the bare indices, so
    the order under a given torch seed (or `generator`) is the reference DataLoader's.  Segment starts: `rng.randint`, one call per
    video in batch order (the reference's order at num_workers=0); `rng` defaults to the global `np.random`.  Per batch: the ids,
    starts and labels go through a pinned slot in one asynchronous copy, one `acx_sample_segments` launch fills a fresh tensor on
    the current stream; the host never waits for the device.

    `bank` needs `paths`, `num_frames`, `file_frames`, `labels_host`, `ncrops` on the host to build the index stream
    (`host_batches`) and `bank`, `row_off`, `frames`, `device` to iterate."""

    already_sharded = True           # Trainer._shard_loader: this iterable yields the calling rank's shard itself
    _SLOTS = 8                       # pinned index slots in rotation (a slot is reused seven batches later)

    def __init__(self, bank, video_ids: Sequence[int], batch_size: int, num_segments: int, seg_length: int, stride: int = 1,
                 shuffle: bool = True, drop_last: bool = True, rng=None, generator: Optional[torch.Generator] = None):
        self.bank = bank
        self.video_ids = np.asarray(list(video_ids), dtype=np.int64)
        self.batch_size, self.N, self.L, self.stride = int(batch_size), int(num_segments), int(seg_length), int(stride)
        self.shuffle, self.drop_last, self.rng, self.generator = bool(shuffle), bool(drop_last), rng, generator
        if min(self.batch_size, self.N, self.L, self.stride) <= 0:
            raise ValueError("ResidentTrainLoader: batch_size, num_segments, seg_length and stride must be positive")
        if len(self.video_ids) and (self.video_ids.min() < 0 or self.video_ids.max() >= len(bank.paths)):
            raise ValueError("ResidentTrainLoader: video_ids outside the bank")
        for v in self.video_ids:
            T = bank.num_frames[v]
            dist, high = FI.train_draw_range(T, self.N, self.L, self.stride)
            if high <= 0:
                raise ValueError(f"{bank.paths[v]}: {T} frames cannot be sampled on a {self.N} x {self.L} segment grid (stride "
                                 f"{self.stride}): the random offset range is {high} (the reference's dataset fails on this "
                                 f"video in np.random.randint)")
            if (self.N - 1) * dist + high >= 2 ** 31:
                raise ValueError(f"{bank.paths[v]}: segment starts do not fit 32 bits")
        self._epoch = 0
        self._shard_seed: Optional[int] = None
        self._index_loader = None
        self._pinned: List[torch.Tensor] = []
        self._copied: List[Optional[torch.cuda.Event]] = []
        self._turn = 0

    # ---- host side: the index stream
    def _order(self):
        """the DataLoader over bare indices whose batches are this rank's video order"""
        from torch.utils.data import DataLoader, DistributedSampler
        ds = _Indices(len(self.video_ids))
        if parallel.is_distributed():
            if self._index_loader is None:
                sampler = DistributedSampler(ds, num_replicas=parallel.world_size(), rank=parallel.rank(), shuffle=self.shuffle,
                                             seed=self._seed())
                self._index_loader = DataLoader(ds, batch_size=self.batch_size, sampler=sampler, drop_last=self.drop_last,
                                                collate_fn=list, generator=self.generator)
            self._index_loader.sampler.set_epoch(self._epoch)
        elif self._index_loader is None:
            self._index_loader = DataLoader(ds, batch_size=self.batch_size, shuffle=self.shuffle, drop_last=self.drop_last,
                                            collate_fn=list, generator=self.generator)
        return self._index_loader

    def _seed(self) -> int:
        """the DistributedSampler seed every rank agrees on, chosen the way Trainer._shard_loader chooses it: PL_GLOBAL_SEED, else
        rank 0's torch seed shared once per loader"""
        if self._shard_seed is None:
            seed = os.environ.get("PL_GLOBAL_SEED")
            if seed is None:
                import torch.distributed as dist
                t = torch.tensor([torch.initial_seed() % (1 << 31)], dtype=torch.int64)
                if dist.get_backend() == "nccl":
                    t = t.cuda()
                dist.broadcast(t, 0)
                seed = int(t.item())
            self._shard_seed = int(seed)
        return self._shard_seed

    def set_epoch(self, epoch: int) -> None:
        self._epoch = int(epoch)

    def __len__(self) -> int:
        return len(self._order())

    def host_batches(self) -> Iterator[Tuple[np.ndarray, np.ndarray, np.ndarray]]:
        """(vid int32 [b] -- indices into the bank --, starts int32 [b * N], labels int64 [b]) per batch: everything a batch is,
        short of the rows.  Draws from the samplers and from `rng` as it goes."""
        bank = self.bank
        for idx in self._order():
            vid = self.video_ids[np.asarray(idx, dtype=np.int64)]
            starts = np.concatenate([FI.train_start_indices(bank.num_frames[v], self.N, self.L, self.stride, self.rng) for v in vid])
            yield vid.astype(np.int32), starts.astype(np.int32), bank.labels_host[vid]

    # ---- device side
    def _slot(self, nbytes: int):
        if not self._pinned:
            self._pinned = [torch.empty(self.batch_size * (12 + 4 * self.N), dtype=torch.uint8).pin_memory() for _ in range(self._SLOTS)]
            self._copied = [None] * self._SLOTS
        k = self._turn
        self._turn = (k + 1) % self._SLOTS
        ev = self._copied[k]
        if ev is not None and not ev.query():       # seven batches behind: only a consumer that never launches anything gets here
            ev.synchronize()
        return k, self._pinned[k][:nbytes]

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        bank, N = self.bank, self.N
        for vid, starts, labels in self.host_batches():
            b = len(vid)
            # one slot, one copy: labels int64 [b] | vid int32 [b] | starts int32 [b * N]
            k, host = self._slot(b * (12 + 4 * N))
            h = host.numpy()
            h[:8 * b].view(np.int64)[:] = labels
            h[8 * b:12 * b].view(np.int32)[:] = vid
            h[12 * b:].view(np.int32)[:] = starts
            with torch.cuda.device(bank.device):
                dev = host.to(bank.device, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                self._copied[k] = ev
                feats = ops.sample_segments(bank.bank, bank.row_off, bank.frames, dev[8 * b:12 * b].view(torch.int32),
                                            dev[12 * b:].view(torch.int32), N, self.L, self.stride, bank.ncrops)
            yield feats, dev[:8 * b].view(torch.int64)
