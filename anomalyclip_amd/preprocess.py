"""CLIP frame preprocessing on the GPU.

Reference: `get_augmentations` (src/utils/augmentations.py:21-34) = GroupScale(224, BICUBIC) -> GroupCenterCrop(224)
-> GroupToTensor -> GroupNormalize(CLIP mean/std); on PIL images torchvision's Resize is `PIL.Image.resize`, i.e.
Pillow's two-pass 8-bit resampler (horizontal then vertical, 22-bit fixed-point coefficients, 8-bit intermediate).
The coefficient tables are computed here on the host in double precision exactly as Pillow's `precompute_coeffs` /
`normalize_coeffs_8bpc` do (published algorithm of libImaging/Resample.c); the device kernels apply them.
JPEG decoding is Pillow's on the host by default; anomalyclip_amd/jpeg.py moves all of it but the Huffman decoding to the device."""
from __future__ import annotations

import ctypes as C
from functools import lru_cache

import numpy as np
import torch

from . import _lib as L
from . import ops
from . import resample as _R

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)      # augmentations.py:23
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)      # augmentations.py:24
_PRECISION_BITS = _R.PRECISION_BITS


def _coeffs(in_size: int, out_size: int):
    """Pillow precompute_coeffs(inSize, 0, inSize, outSize, BICUBIC) + normalize_coeffs_8bpc (anomalyclip_amd/resample.py)."""
    return _R.coeffs(in_size, out_size, "bicubic")


def resize_geometry(h: int, w: int, size: int):
    """torchvision Resize(size) on (h, w): shorter side -> size (int truncation), then CenterCrop(size) offsets."""
    if w <= h:
        ow, oh = size, int(size * h / w)
    else:
        oh, ow = size, int(size * w / h)
    top = int(round((oh - size) / 2.0))
    left = int(round((ow - size) / 2.0))
    return oh, ow, top, left


@lru_cache(maxsize=16)
def _tables(h: int, w: int, size: int, device_str: str):
    oh, ow, top, left = resize_geometry(h, w, size)
    hb, hk, hks = _coeffs(w, ow)
    vb, vk, vks = _coeffs(h, oh)
    dev = torch.device(device_str)
    sl_h, sl_v = slice(left, left + size), slice(top, top + size)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t(hb[sl_h]), t(hk[sl_h]), hks, t(vb[sl_v]), t(vk[sl_v]), vks


def preprocess_frames(frames_u8: torch.Tensor, size: int = 224, mean=CLIP_MEAN, std=CLIP_STD) -> torch.Tensor:
    """frames_u8: [F, H, W, 3] uint8 on the device -> [F, 3, size, size] float32 (the ViT's input)."""
    assert frames_u8.dtype == torch.uint8 and frames_u8.dim() == 4 and frames_u8.shape[-1] == 3 and frames_u8.is_contiguous()
    F, H, W, _ = frames_u8.shape
    hb, hk, hks, vb, vk, vks = _tables(H, W, size, str(frames_u8.device))
    out = torch.empty(F, 3, size, size, dtype=torch.float32, device=frames_u8.device)
    tmp = torch.empty(F, H, size, 3, dtype=torch.uint8, device=frames_u8.device)
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    h = ops._h(frames_u8)
    L.check(L.lib().acx_preprocess_frames(h, frames_u8.data_ptr(), out.data_ptr(), tmp.data_ptr(), hb.data_ptr(), hk.data_ptr(),
                                          hks, vb.data_ptr(), vk.data_ptr(), vks, F, H, W, size, size, m, s, ops._stream()), h)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Multi-crop front end: GroupScale(scale_size) -> CenterCrop / FiveCrop / TenCrop(crop_size) -> ToTensor -> Normalize
# (reference gtransforms.py:89-102, 449-477; the crops are torchvision's published five_crop / ten_crop).
def scaled_size(h: int, w: int, scale_size: int):
    """(oh, ow) of Resize(scale_size) on (h, w): the shorter side becomes scale_size, the other int(scale_size * long / short)"""
    if w <= h:
        return int(scale_size * h / w), scale_size
    return scale_size, int(scale_size * w / h)


def default_scale_size(crop_size: int, ncrops: int) -> int:
    """one crop: the reference's transform (scale == crop); 5 / 10 crops: the usual 8 / 7 (256 for 224, 384 for 336)"""
    return crop_size if ncrops == 1 else crop_size * 8 // 7


def crop_windows(h: int, w: int, scale_size: int, crop_size: int, ncrops: int):
    """The crops of an (h, w) frame as windows of its resized image: [(top, left, flip)] in output order, `top` / `left` in
    rows / columns of the resized image.  flip: the crop belongs to the horizontally mirrored image -- its window (t, l) there is
    columns ow - C - l .. of the unmirrored image, read right to left; `left` is already that unmirrored column.
    1: centre.  5: tl, tr, bl, br, centre.  10: those five, then the same five of the mirrored image."""
    if ncrops not in (1, 5, 10):
        raise ValueError(f"ncrops must be 1, 5 or 10, not {ncrops!r}")
    if scale_size < crop_size:
        raise ValueError(f"scale_size {scale_size} is smaller than crop_size {crop_size}")
    oh, ow = scaled_size(h, w, scale_size)
    C_ = crop_size
    centre = (int(round((oh - C_) / 2.0)), int(round((ow - C_) / 2.0)))
    if ncrops == 1:
        return [(centre[0], centre[1], False)]
    five = [(0, 0), (0, ow - C_), (oh - C_, 0), (oh - C_, ow - C_), centre]
    wins = [(t, l, False) for t, l in five]
    if ncrops == 10:
        wins += [(t, ow - C_ - l, True) for t, l in five]
    return wins


@lru_cache(maxsize=16)
def _full_tables(h: int, w: int, scale_size: int, device_str: str):
    """the tables of the WHOLE resized image (every crop is a window of them)"""
    oh, ow = scaled_size(h, w, scale_size)
    hb, hk, hks = _coeffs(w, ow)
    vb, vk, vks = _coeffs(h, oh)
    dev = torch.device(device_str)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return oh, ow, t(hb), t(hk), hks, t(vb), t(vk), vks


def preprocess_crops(frames_u8: torch.Tensor, crop_size: int, scale_size=None, ncrops: int = 1, mean=CLIP_MEAN,
                     std=CLIP_STD, out=None) -> torch.Tensor:
    """frames_u8: [F, H, W, 3] uint8 on the device -> [F, ncrops, 3, crop_size, crop_size] float32: image f * ncrops + c is crop c
    of frame f (the row order of a feature file).  One library call for all crops of all frames.  out: a contiguous float32
    tensor of F * ncrops images of the same device to write them into (a slice of a larger input batch); it is returned viewed
    as [F, ncrops, 3, crop_size, crop_size]."""
    assert frames_u8.dtype == torch.uint8 and frames_u8.dim() == 4 and frames_u8.shape[-1] == 3 and frames_u8.is_contiguous()
    if scale_size is None:
        scale_size = default_scale_size(crop_size, ncrops)
    F, H, W, _ = frames_u8.shape
    wins = crop_windows(H, W, scale_size, crop_size, ncrops)
    oh, ow, hb, hk, hks, vb, vk, vks = _full_tables(H, W, scale_size, str(frames_u8.device))
    if out is None:
        out = torch.empty(F, ncrops, 3, crop_size, crop_size, dtype=torch.float32, device=frames_u8.device)
    else:
        if (out.dtype != torch.float32 or out.device != frames_u8.device or not out.is_contiguous()
                or out.numel() != F * ncrops * 3 * crop_size * crop_size or out.data_ptr() % 16):
            raise ValueError(f"preprocess_crops: out must be contiguous float32 on {frames_u8.device}, 16-byte aligned, of "
                             f"{F * ncrops} images 3 x {crop_size} x {crop_size}; got {tuple(out.shape)} {out.dtype} on {out.device}")
        out = out.view(F, ncrops, 3, crop_size, crop_size)
    tmp = torch.empty(F, H, ow, 3, dtype=torch.uint8, device=frames_u8.device)
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    wv = (C.c_int32 * (3 * ncrops))(*[int(v) for win in wins for v in win])
    h = ops._h(frames_u8)
    L.check(L.lib().acx_preprocess_crops(h, frames_u8.data_ptr(), out.data_ptr(), tmp.data_ptr(), hb.data_ptr(), hk.data_ptr(),
                                         hks, vb.data_ptr(), vk.data_ptr(), vks, F, H, W, oh, ow, crop_size, ncrops, wv, m, s,
                                         ops._stream()), h)
    return out
