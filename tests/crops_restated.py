"""Test infrastructure for the multi-crop front end: GroupScale -> CenterCrop / FiveCrop / TenCrop restated with Pillow alone
(torchvision is not installed; on PIL images its Resize is `Image.resize`, its crops are `Image.crop`, its hflip is
`Image.transpose(FLIP_LEFT_RIGHT)`), plus a numpy evaluation of the package's coefficient tables, sliced and mirrored per crop."""
import numpy as np
import torch
from PIL import Image

MEAN = np.array([0.48145466, 0.4578275, 0.40821073], dtype=np.float32)
STD = np.array([0.26862954, 0.26130258, 0.27577711], dtype=np.float32)

GEOMETRIES = [(240, 320, 256, 224), (241, 323, 256, 224), (360, 201, 256, 224), (120, 160, 256, 224), (97, 131, 36, 32),
              (480, 856, 384, 336), (224, 224, 224, 224)]           # (H, W, scale_size, crop_size)


def _scale(img, size):
    w, h = img.size
    if w <= h:
        ow, oh = size, int(size * h / w)
    else:
        oh, ow = size, int(size * w / h)
    return img.resize((ow, oh), Image.BICUBIC)


def _center(img, c):
    w, h = img.size
    top, left = int(round((h - c) / 2.0)), int(round((w - c) / 2.0))
    return img.crop((left, top, left + c, top + c))


def _five(img, c):
    w, h = img.size
    return [img.crop((0, 0, c, c)), img.crop((w - c, 0, w, c)), img.crop((0, h - c, c, h)), img.crop((w - c, h - c, w, h)),
            _center(img, c)]


def _crops(img, c, ncrops):
    if ncrops == 1:
        return [_center(img, c)]
    if ncrops == 5:
        return _five(img, c)
    assert ncrops == 10
    return _five(img, c) + _five(img.transpose(Image.FLIP_LEFT_RIGHT), c)


def pil_crops(frame_u8, scale_size, crop_size, ncrops):
    """[H, W, 3] uint8 -> [ncrops, C, C, 3] uint8 through Pillow"""
    img = _scale(Image.fromarray(np.asarray(frame_u8)), scale_size)
    return np.stack([np.asarray(c) for c in _crops(img, crop_size, ncrops)])


def pil_windows(h, w, scale_size, crop_size, ncrops):
    """[(top, left, flip)] read off what Pillow's crop / transpose do to an image whose pixels hold their own position"""
    if w <= h:
        ow, oh = scale_size, int(scale_size * h / w)
    else:
        oh, ow = scale_size, int(scale_size * w / h)
    pos = Image.fromarray(np.arange(oh * ow, dtype=np.int32).reshape(oh, ow))
    out = []
    for c in _crops(pos, crop_size, ncrops):
        a = np.asarray(c)
        assert a.shape == (crop_size, crop_size)
        y, x0, x1 = int(a[0, 0]) // ow, int(a[0, 0]) % ow, int(a[0, -1]) % ow
        flip = x1 < x0 if crop_size > 1 else False
        left = x1 if flip else x0
        want = (np.arange(y, y + crop_size)[:, None] * ow + (np.arange(left, left + crop_size)[::-1] if flip
                                                             else np.arange(left, left + crop_size))[None, :])
        assert np.array_equal(a, want)                      # the crop IS that window, whole
        out.append((y, left, flip))
    return out


def normalise(u8):
    """[..., C, C, 3] uint8 -> [..., 3, C, C] float32: ToTensor (/255), Normalize(CLIP mean, std)"""
    t = torch.from_numpy(np.asarray(u8).astype(np.float32) / np.float32(255.0)).movedim(-1, -3)
    return (t - torch.from_numpy(MEAN).view(3, 1, 1)) / torch.from_numpy(STD).view(3, 1, 1)


def pil_crops_float(frames_u8, scale_size, crop_size, ncrops):
    """[F, H, W, 3] uint8 -> [F, ncrops, 3, C, C] float32, the expected output of preprocess_crops"""
    return torch.stack([normalise(pil_crops(f, scale_size, crop_size, ncrops)) for f in np.asarray(frames_u8)])


def _clip8(acc):
    return np.clip(acc >> 22, 0, 255).astype(np.uint8)


def table_crops(frame_u8, scale_size, crop_size, ncrops):
    """The same crops from the package's tables: for each window of preprocess.crop_windows, the rows top .. and the columns
    left .. of the full tables (reversed when flipped), applied horizontally then vertically in 8-bit fixed point."""
    from anomalyclip_amd import preprocess as P
    f = np.asarray(frame_u8).astype(np.int64)
    H, W, _ = f.shape
    oh, ow = P.scaled_size(H, W, scale_size)
    hb, hk, _ = P._coeffs(W, ow)
    vb, vk, _ = P._coeffs(H, oh)
    out = []
    for top, left, flip in P.crop_windows(H, W, scale_size, crop_size, ncrops):
        cols = np.arange(left, left + crop_size)
        cols = cols[::-1] if flip else cols
        tmp = np.empty((H, crop_size, 3), dtype=np.int64)
        for j, xi in enumerate(cols):
            x0, n = hb[xi]
            tmp[:, j] = _clip8((f[:, x0:x0 + n] * hk[xi, :n].astype(np.int64)[None, :, None]).sum(1) + (1 << 21))
        img = np.empty((crop_size, crop_size, 3), dtype=np.uint8)
        for i in range(crop_size):
            y0, n = vb[top + i]
            img[i] = _clip8((tmp[y0:y0 + n] * vk[top + i, :n].astype(np.int64)[:, None, None]).sum(0) + (1 << 21))
        out.append(img)
    return np.stack(out)


def make_frames(h, w, n=2, seed=0):
    """seeded frames with saturated and flat regions (the clip8 paths)"""
    g = torch.Generator().manual_seed(seed * 100003 + h * 131 + w)
    fr = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    fr[0, : h // 2] = 255
    if n > 1:
        fr[1, :, : w // 3] = 0
    return fr

