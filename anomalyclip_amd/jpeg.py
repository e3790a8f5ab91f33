"""Baseline JPEG frames decoded on the GPU, bit for bit Pillow's `Image.open(p).convert("RGB")`.

The decoder is split where the work changes character.  Huffman decoding is sequential and driven by untrusted bytes: it runs on the
host (`acx_jpeg_parse` + `acx_jpeg_entropy_decode`, called through ctypes with the GIL released, one frame per pool thread) and
leaves every block's 64 coefficients, de-zigzagged and not dequantised, in a pinned buffer.  Dequantisation, the inverse DCT, chroma
upsampling and the colour conversion are regular integer arithmetic over every sample: `ops.jpeg_reconstruct` does them on the
device for a whole batch, into the uint8 [k, H, W, 3] tensor `preprocess_crops` takes.

`JpegFolderReader` is `extract.FrameFolderReader` with that decoder: same folder conventions, same interface, but its batches are
DEVICE tensors.  A file the host decoder does not take (progressive, CMYK, subsampled and at most 4 pixels wide, PNG under a `.jpg`
template, damaged, of another sampling than the video's leading frames ...) is decoded by Pillow in the same worker and copied into its place, so every frame is
Pillow's either way; `fallbacks` counts them.

`JpegEntropyFolderReader` (`decode="gpu_entropy"`) moves the Huffman decoding to the device as well: the pool threads only read the
files, walk their markers and un-stuff their scans (`acx_jpeg_scan_pack`) into a pinned buffer, and `ops.jpeg_entropy_decode` decodes
the whole batch in one launch, one workgroup per frame, into the coefficient buffer `ops.jpeg_reconstruct` takes.  What crosses to
the device is the file's size, not its coefficients'."""
from __future__ import annotations

import ctypes as C
import os
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Iterator, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from . import ops
from .extract import TEMPLATE, FrameFolderReader

DECODERS = ("pil", "gpu", "gpu_entropy")
E_UNSUPPORTED = -2                     # ACX_E_UNSUPPORTED
GEOMETRY_PROBES = 4                    # leading frames looked at for the video's sampling before the whole video goes to Pillow


def check_decode(decode, key: str = "decode") -> str:
    """the `decode` switch of extract / extract_dataset / FeatureBank.from_frames / AnomalyCLIPDataModule"""
    if decode not in DECODERS:
        raise ValueError(f"{key}={decode!r}: the frame decoder is 'pil' (Pillow on the host), 'gpu' (baseline JPEG, reconstructed "
                         f"on the device) or 'gpu_entropy' (its Huffman decoding on the device too)")
    return decode


def make_reader(decode: str, frames_root: str, video: str, start=None, end=None, template: str = TEMPLATE, threads: int = 8):
    """the frame reader of a video for `decode`: extract.FrameFolderReader ('pil'), JpegFolderReader ('gpu') or
    JpegEntropyFolderReader ('gpu_entropy')"""
    from . import extract as X
    if check_decode(decode) != "pil":
        return READERS[decode](frames_root, video, start, end, template, threads)
    return X.FrameFolderReader(frames_root, video, start, end, template, threads)


def parse(data: bytes) -> Tuple[int, L.JpegInfo]:
    """(return code, acx_jpeg_info) of a JPEG file's bytes"""
    info = L.JpegInfo()
    rc = L.lib().acx_jpeg_parse(data, len(data), C.byref(info))
    return rc, info


def geometry_of(info: L.JpegInfo) -> Tuple[int, int, int, int, int]:
    """(H, W, ncomp, hs, vs): what frames must share to be reconstructed in one launch"""
    return int(info.height), int(info.width), int(info.ncomp), int(info.comp_h[0]), int(info.comp_v[0])


class JpegFolderReader(FrameFolderReader):
    """`FrameFolderReader` whose `batches(n)` yields (slot, uint8 [k, H, W, 3]) DEVICE tensors: files are read and entropy-decoded
    on the pool into two pinned coefficient buffers in rotation, one batch ahead of the consumer; the copy to the device and the
    two reconstruction kernels run on a side stream, and the stream that is current when a batch is taken waits for them.  Every
    batch is a fresh tensor (allocated on the side stream, `record_stream`ed for the consumer's), so the consumer holds no buffer of
    the reader's: `copied` is kept for the interface only."""

    def __init__(self, frames_root: str, video: str, start: Optional[int] = None, end: Optional[int] = None,
                 template: str = TEMPLATE, threads: int = 8, device: Optional[torch.device] = None):
        super().__init__(frames_root, video, start, end, template, threads, pinned=True)
        self._init_state(device)

    @classmethod
    def like(cls, reader: FrameFolderReader, device=None) -> "JpegFolderReader":
        """the frames of `reader` (a FrameFolderReader that has not been read yet), decoded this way"""
        self = cls.__new__(cls)
        self.dir, self.template, self.indices = reader.dir, reader.template, list(reader.indices)
        self._init_reader(reader.threads, pinned=True)
        self._init_state(device)
        return self

    def _init_state(self, device):
        self.device = device
        self.fallbacks = 0                 # frames Pillow decoded
        self._geom = None                  # (H, W, ncomp, hs, vs) of the first of the video's leading frames the host decoder takes;
                                           # False: it takes none of them
        self._coef = [None, None]          # per slot: pinned int16 [n, coef_elems]
        self._qt = [None, None]            # per slot: pinned int16 [n, ncomp, 64] (the bits of uint16)
        self._rgb = [None, None]           # per slot: pinned uint8 [n, H, W, 3] for Pillow's frames, allocated at the first one
        self._done = [None, None]          # per slot: the event after the copies that READ the pinned buffers
        self._side = None
        self._lock = threading.Lock()
        self._turn = 0                     # decode_into: the slot of the next piece

    device_frames = True                   # decode_into / finish_into leave the frames in a DEVICE tensor of the caller's

    def borrow(self, pool: ThreadPoolExecutor, side=None) -> None:
        """FrameFolderReader.borrow; the copies and the decoder's kernels go on the lender's `side` stream"""
        super().borrow(pool)
        if side is not None:
            self._side = side

    # ------------------------------------------------------------------------------------------------------------ host
    @property
    def geometry(self):
        """(H, W, ncomp, hs, vs) of the first of the video's GEOMETRY_PROBES leading frames that the host decoder takes and whose
        size is the video's; None if there is none: every frame of such a video (PNG frames, all progressive) is Pillow's"""
        if self._geom is None:
            self._geom = False
            size = self.frame_size
            for i in range(min(len(self), GEOMETRY_PROBES)):
                try:
                    with open(self.path(i), "rb") as fh:
                        rc, info = parse(fh.read())
                except FileNotFoundError:
                    continue
                if rc == 0 and geometry_of(info)[:2] == size:
                    self._geom = geometry_of(info)
                    break
        return self._geom or None

    def _pillow(self, i: int, j: int, slot: int, n: int):
        """frame i of the folder as Pillow decodes it, into place j of the slot's RGB buffer"""
        H, W = self.frame_size
        with self._lock:
            if self._rgb[slot] is None or self._rgb[slot].shape[0] < n:
                self._rgb[slot] = torch.empty(n, H, W, 3, dtype=torch.uint8).pin_memory()
            self.fallbacks += 1
        FrameFolderReader._decode(self, i, self._rgb[slot][j].numpy())

    def _entropy(self, i: int, j: int, slot: int, n: int, coef: np.ndarray, qt: np.ndarray) -> bool:
        """frame i into coef[j], qt[j]; False: Pillow decoded it instead"""
        geom = self.geometry
        if geom is not None:
            with open(self.path(i), "rb") as fh:
                data = fh.read()
            rc, info = parse(data)
            if rc == 0 and geometry_of(info) == geom:
                row = coef[j]
                row.fill(0)
                rc = L.lib().acx_jpeg_entropy_decode(data, len(data), C.byref(info), row.ctypes.data, row.size)
                if rc == 0:
                    for c in range(geom[2]):
                        qt[j, c] = np.ctypeslib.as_array(info.qtab[int(info.comp_tq[c])])
                    return True
        self._pillow(i, j, slot, n)
        return False

    def _fill(self, i0: int, i1: int, slot: int):
        n = i1 - i0
        if self._done[slot] is not None:              # the copies that read this slot's buffers two batches ago must be over
            self._done[slot].synchronize()
            self._done[slot] = None
        geom = self.geometry
        coef = qt = None
        if geom is not None:
            elems = ops.jpeg_coef_elems(*geom)
            if self._coef[slot] is None or self._coef[slot].shape[0] < n:
                self._coef[slot] = torch.empty(n, elems, dtype=torch.int16).pin_memory()
                self._qt[slot] = torch.zeros(n, geom[2], 64, dtype=torch.int16).pin_memory()
            coef, qt = self._coef[slot][:n].numpy(), self._qt[slot][:n].numpy().view(np.uint16)
        ok = list(self.pool().map(lambda j: self._entropy(i0 + j, j, slot, n, coef, qt), range(n)))
        return n, ok

    def decode_batch(self, i0: int, i1: int, slot: int):
        """the host stage of one batch, on its own (measurements): frames i0 ... i1 - 1 entropy-decoded into the slot's pinned
        buffers -> (coef int16 [n, coef_elems], qtabs int16 [n, ncomp, 64], per frame: False where Pillow decoded it)"""
        n, ok = self._fill(i0, i1, slot)
        if self._coef[slot] is None:
            return None, None, ok
        return self._coef[slot][:n], self._qt[slot][:n], ok

    def decode_into(self, i0: int, i1: int, dst: torch.Tensor):
        """the host stage of frames i0 ... i1 - 1, meant for the caller's DEVICE uint8 [i1 - i0, H, W, 3] `dst` (a slice of a
        launch that holds other videos' frames too): on the thread that decodes ahead, through this reader's two slots of
        pinned buffers in rotation.  -> what finish_into takes, on the consumer's thread, at most one piece later"""
        assert dst.is_cuda and dst.dtype == torch.uint8 and dst.shape == (i1 - i0, *self.frame_size, 3) and dst.is_contiguous()
        slot, self._turn = self._turn, self._turn ^ 1
        return (slot, dst) + tuple(self._fill(i0, i1, slot))

    def finish_into(self, token) -> torch.Tensor:
        """the device stage of decode_into's piece: its frames are in `dst` for the current stream"""
        slot, dst, n, ok = token
        return self._launch(slot, n, ok, out=dst)

    # ------------------------------------------------------------------------------------------------------------ device
    def _launch(self, slot: int, n: int, ok, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the batch in the slot's pinned buffers -> uint8 [n, H, W, 3] on the device (`out`, if the caller has a place for it),
        ready for the current stream"""
        dev = torch.device("cuda", torch.cuda.current_device()) if self.device is None else torch.device(self.device)
        H, W = self.frame_size
        cur = torch.cuda.current_stream(dev)
        if self._side is None:
            self._side = torch.cuda.Stream(device=dev)
        with torch.cuda.device(dev), torch.cuda.stream(self._side):
            if out is None:
                out = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
            if any(ok):
                coef = self._coef[slot][:n].to(dev, non_blocking=True)
                qt = self._qt[slot][:n].to(dev, non_blocking=True)
                ops.jpeg_reconstruct(coef, qt, *self.geometry, out=out)
            for j in range(n):
                if not ok[j]:                         # (after the kernels, which wrote this frame from whatever its row held)
                    out[j].copy_(self._rgb[slot][j], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._side)
        self._done[slot] = ev
        cur.wait_event(ev)
        out.record_stream(cur)
        return out

    def batches(self, n: int) -> Iterator[Tuple[int, torch.Tensor]]:
        """(slot, uint8 [k, H, W, 3] on the device) for consecutive groups of n frames; batch k + 1 is being entropy-decoded while
        k is reconstructed and consumed"""
        if not torch.cuda.is_available():
            raise L.AcxError("JpegFolderReader reconstructs its frames on the GPU (no CPU fallback); decode='pil' reads them on the host")
        T = len(self)
        spans = [(i, min(T, i + n)) for i in range(0, T, n)]
        with ThreadPoolExecutor(max_workers=1) as driver:
            try:
                fut = driver.submit(self._fill, *spans[0], 0)
                for k in range(len(spans)):
                    cnt, ok = fut.result()
                    fut = driver.submit(self._fill, *spans[k + 1], (k + 1) & 1) if k + 1 < len(spans) else None
                    yield k & 1, self._launch(k & 1, cnt, ok)
            finally:
                self.close()
                for ev in self._done:                 # the pinned buffers go with the reader: not before their last copy
                    if ev is not None:
                        ev.synchronize()


class JpegEntropyFolderReader(JpegFolderReader):
    """`JpegFolderReader` whose Huffman decoding runs on the device too.  The pool threads read, parse and pack the scans into two
    pinned buffers in rotation; the reader's DRIVER thread (the one that fills the batch ahead) puts the copies, the zeroing of the
    coefficients, the entropy kernel and the reconstruction on the side stream, waits for the per-frame status to come back, and has
    Pillow decode every frame whose status is not 0 -- the consumer's thread only makes its stream wait for the finished batch.  A
    file with a restart interval is the host decoder's (`acx_jpeg_entropy_decode`, then Pillow if that fails too); a file the parser
    refuses or of another geometry is Pillow's, as in the parent."""

    SCAN_ALIGN = 16                                   # a frame's first byte in the batch's scan buffer (a multiple of ops.JPEG_SCAN_ALIGN)

    def _init_state(self, device):
        super()._init_state(device)
        self._scan = [None, None]          # per slot: pinned uint8, the packed scans of a batch one after the other
        self._meta = [None, None]          # per slot: pinned (scan_off int64 [n], scan_bits int32 [n], huff uint8 [n, HUFF], status int32 [n])
        self.h2d_bytes = 0                 # bytes copied to the device so far (measurements)
        self.sub_bits = 0                  # bits per subsequence; 0: each frame's smallest

    # ------------------------------------------------------------------------------------------------------------ host
    def _pack(self, i: int, j: int, slot: int, n: int, scan: np.ndarray, off: int, cap: int, meta, qt: np.ndarray, host) -> int:
        """frame i: its scan into scan[off : off + cap], its tables into row j.  1: the device decodes it; 2: the host decoder did
        (a restart interval), into the slot's pinned coefficients; 0: Pillow did"""
        geom = self.geometry
        with open(self.path(i), "rb") as fh:
            data = fh.read()
        rc, info = parse(data)
        if rc == 0 and geometry_of(info) == geom:
            rc, nbytes = ops.jpeg_scan_pack(data, info, scan[off:off + cap], meta[2][j])
            if rc == 0:
                meta[0][j] = off * 8
                meta[1][j] = nbytes * 8
                for c in range(geom[2]):
                    qt[j, c] = np.ctypeslib.as_array(info.qtab[int(info.comp_tq[c])])
                return 1
            if rc == E_UNSUPPORTED:
                coef = host()
                return 2 if self._entropy(i, j, slot, n, coef, qt) else 0
        self._pillow(i, j, slot, n)
        return 0

    def _host_coef(self, slot: int, n: int) -> np.ndarray:
        """the slot's pinned coefficients for the frames the host decoder takes, allocated at the first of them"""
        with self._lock:
            if self._coef[slot] is None or self._coef[slot].shape[0] < n:
                self._coef[slot] = torch.empty(n, ops.jpeg_coef_elems(*self.geometry), dtype=torch.int16).pin_memory()
            return self._coef[slot][:n].numpy()

    def _pack_batch(self, i0: int, i1: int, slot: int):
        """the host stage: -> (n, per frame 1 / 2 / 0 as _pack returns, bytes of the scan buffer in use)"""
        n = i1 - i0
        if self._done[slot] is not None:              # the copies that read this slot's buffers two batches ago must be over
            self._done[slot].synchronize()
            self._done[slot] = None
        geom = self.geometry
        if geom is None:
            list(self.pool().map(lambda j: self._pillow(i0 + j, j, slot, n), range(n)))
            return n, [0] * n, 0
        caps = [-(-os.path.getsize(self.path(i0 + j)) // self.SCAN_ALIGN) * self.SCAN_ALIGN for j in range(n)]   # a scan is shorter than its file
        offs = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
        total = int(offs[-1])
        if self._scan[slot] is None or self._scan[slot].numel() < total:
            self._scan[slot] = torch.empty(max(total + total // 4, 1 << 16), dtype=torch.uint8).pin_memory()
        if self._meta[slot] is None or self._meta[slot][0].shape[0] < n:
            self._meta[slot] = (torch.zeros(n, dtype=torch.int64).pin_memory(), torch.zeros(n, dtype=torch.int32).pin_memory(),
                                torch.zeros(n, ops.JPEG_HUFF_BYTES, dtype=torch.uint8).pin_memory(),
                                torch.zeros(n, dtype=torch.int32).pin_memory())
            self._qt[slot] = torch.zeros(n, geom[2], 64, dtype=torch.int16).pin_memory()
        meta = [m[:n].numpy() for m in self._meta[slot]]
        meta[0][:] = 0                                # a frame the device does not decode is an empty scan: a status, no more
        meta[1][:] = 0
        scan, qt = self._scan[slot].numpy(), self._qt[slot][:n].numpy().view(np.uint16)
        host = lambda: self._host_coef(slot, n)
        how = list(self.pool().map(lambda j: self._pack(i0 + j, j, slot, n, scan, int(offs[j]), caps[j], meta, qt, host), range(n)))
        return n, how, total

    def decode_batch(self, i0: int, i1: int, slot: int):
        """the host stage of one batch, on its own (measurements): frames i0 ... i1 - 1 read, parsed and packed into the slot's pinned
        buffers -> (scans uint8 [bytes], (scan_off, scan_bits, huff), per frame: 1 where the device is to decode it)"""
        n, how, total = self._pack_batch(i0, i1, slot)
        if self._scan[slot] is None:
            return None, None, how
        return self._scan[slot][:total], tuple(m[:n] for m in self._meta[slot][:3]), how

    # ------------------------------------------------------------------------------------------------------------ device
    def decode_into(self, i0: int, i1: int, dst: torch.Tensor):
        """JpegFolderReader.decode_into; here the thread that decodes ahead puts the piece's device work on the side stream too"""
        assert dst.is_cuda and dst.dtype == torch.uint8 and dst.shape == (i1 - i0, *self.frame_size, 3) and dst.is_contiguous()
        slot, self._turn = self._turn, self._turn ^ 1
        return (slot,) + tuple(self._fill(i0, i1, slot, out=dst))

    def finish_into(self, token) -> torch.Tensor:
        return self._launch(*token)

    def _fill(self, i0: int, i1: int, slot: int, out: Optional[torch.Tensor] = None):
        """on the driver thread: the host stage, then the batch's whole device work on the side stream -> (out, event)"""
        n, how, total = self._pack_batch(i0, i1, slot)
        dev = torch.device("cuda", torch.cuda.current_device()) if self.device is None else torch.device(self.device)
        H, W = self.frame_size
        if self._side is None:
            self._side = torch.cuda.Stream(device=dev)
        with torch.cuda.device(dev), torch.cuda.stream(self._side):
            if out is None:
                out = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
            pillow = [j for j in range(n) if how[j] == 0]
            if any(how):
                geom = self.geometry
                off_h, bits_h, huff_h, status_h = (m[:n] for m in self._meta[slot])
                scans = self._scan[slot][:max(total, 16)].to(dev, non_blocking=True)
                off, bits, huff = (m.to(dev, non_blocking=True) for m in (off_h, bits_h, huff_h))
                qt = self._qt[slot][:n].to(dev, non_blocking=True)
                self.h2d_bytes += sum(t.numel() * t.element_size() for t in (scans, off, bits, huff, qt))
                coef, status = ops.jpeg_entropy_decode(scans, off, bits, huff, *geom, max_scan_bits=int(bits_h.max()),
                                                       sub_bits=self.sub_bits)
                for j in range(n):
                    if how[j] == 2:                   # the host decoder's frames: their coefficients go where the kernel left zeros
                        coef[j].copy_(self._coef[slot][j], non_blocking=True)
                        self.h2d_bytes += coef[j].numel() * 2
                ops.jpeg_reconstruct(coef, qt, *geom, out=out)
                status_h.copy_(status, non_blocking=True)
                back = torch.cuda.Event()
                back.record(self._side)
                back.synchronize()                    # (this thread's wait: the consumer is busy with the batch before)
                bad = [j for j in range(n) if how[j] == 1 and int(status_h[j]) != 0]
                list(self.pool().map(lambda j: self._pillow(i0 + j, j, slot, n), bad))
                pillow += bad
            for j in pillow:                          # (after the kernels, which wrote these frames from whatever their rows held)
                out[j].copy_(self._rgb[slot][j], non_blocking=True)
                self.h2d_bytes += out[j].numel()
            ev = torch.cuda.Event()
            ev.record(self._side)
        self._done[slot] = ev
        return out, ev

    def _launch(self, slot: int, out: torch.Tensor, ev) -> torch.Tensor:
        """on the consumer's thread, with what _fill returned: the finished batch, ready for the current stream"""
        cur = torch.cuda.current_stream(out.device)
        cur.wait_event(ev)
        out.record_stream(cur)
        return out

    def batches(self, n: int) -> Iterator[Tuple[int, torch.Tensor]]:
        """(slot, uint8 [k, H, W, 3] on the device) for consecutive groups of n frames; batch k + 1 is packed, decoded and
        reconstructed while k is consumed"""
        if not torch.cuda.is_available():
            raise L.AcxError("JpegEntropyFolderReader decodes its frames on the GPU (no CPU fallback); decode='pil' reads them on the host")
        yield from super().batches(n)


READERS = {"gpu": JpegFolderReader, "gpu_entropy": JpegEntropyFolderReader}
