"""Host-side mirror of the reference's CLIP ResNet image encoder (clip/model.py:10-171): same module tree, parameter and buffer
names (every BatchNorm's running_mean / running_var / num_batches_tracked, `downsample.0` / `downsample.1`), so reference and
Lightning checkpoints load with load_state_dict(strict=True); `forward` hands folded weights and raw device pointers to libacx.

Reference mapping
    Bottleneck        clip/model.py:10-68
    AttentionPool2d   clip/model.py:71-108
    ModifiedResNet    clip/model.py:111-171
The encoder is frozen in AnomalyCLIP (anomaly_clip_module.py:68-69), so only a forward exists.  In eval mode every BatchNorm is
folded into its convolution (acx_resnet_encode).  In training mode (Lightning's model.train() reaches the frozen encoder) every
BatchNorm normalises with the batch statistics of all frames of the call and updates its running statistics
(acx_resnet_encode_train), as the reference does.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import List, Optional, Sequence

import torch
from torch import nn

from .. import _lib as L
from .. import ops

# "auto" (the default) and "f32" run the f32 MFMA kernels; "f32x6" is the older name of "auto".  "bf16x6" (opt-in, eval mode) runs
# the convolutions as f32-accurate six-product GEMMs of bf16 planes (ACX_PREC_BF16X6); training mode stays on the f32 kernels.
RESNET_PRECISIONS = {"auto": L.PREC_F32X6, "f32": L.PREC_F32, "f32x6": L.PREC_F32X6, "bf16x6": L.PREC_BF16X6}


def _routed(K: int, conv3x3: bool) -> bool:
    """acx_resnet_encode's routing rule at ACX_PREC_BF16X6 (csrc/acx_resnet.hip rn_routed): the products that read w3 planes"""
    return conv3x3 or K >= 64


def check_resnet_precision(precision: str, arch: str, width: int = 64):
    """A ValueError, before anything is allocated, for a precision the ResNet encoders do not run (or a width they do not take:
    width % 8 == 0 keeps every block's 4 * planes outputs a multiple of 32 channels, as in CLIP's five ResNets)."""
    if width % 8:
        raise ValueError(f"{arch}: width {width} is not a multiple of 8 (acx_resnet_encode)")
    if precision not in RESNET_PRECISIONS:
        raise ValueError(f"precision {precision!r} is not available for {arch}: the ResNet encoders run 'auto', 'f32' or 'bf16x6'")


def _cp(c: int) -> int:
    return (c + 31) // 32 * 32                      # channel count of an NHWC activation (include/acx.h: multiples of 32)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes: int, planes: int, stride: int = 1):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = None
        self.stride = stride
        if stride > 1 or inplanes != planes * 4:
            self.downsample = nn.Sequential(OrderedDict([("-1", nn.AvgPool2d(stride)),
                                                         ("0", nn.Conv2d(inplanes, planes * 4, 1, bias=False)),
                                                         ("1", nn.BatchNorm2d(planes * 4))]))


class AttentionPool2d(nn.Module):
    def __init__(self, spacial_dim: int, embed_dim: int, num_heads: int, output_dim: Optional[int] = None):
        super().__init__()
        self.positional_embedding = nn.Parameter(torch.randn(spacial_dim ** 2 + 1, embed_dim) / embed_dim ** 0.5)
        self.k_proj = nn.Linear(embed_dim, embed_dim)
        self.q_proj = nn.Linear(embed_dim, embed_dim)
        self.v_proj = nn.Linear(embed_dim, embed_dim)
        self.c_proj = nn.Linear(embed_dim, output_dim or embed_dim)
        self.num_heads = num_heads


def _fold(conv: nn.Conv2d, bn: Optional[nn.BatchNorm2d], cin_p: int, stem: bool = False):
    """(w [Cout_p][taps * Cin_p], b [Cout_p]) with the eval BatchNorm folded in, in f64, stored f32 (include/acx.h acx_resnet_conv);
    bn None: the convolution's own weight in that layout, b zero (the training-mode driver normalises the raw product)."""
    w = conv.weight.detach().double()
    cout, cin, k, _ = w.shape
    if bn is None:
        s = torch.ones(cout, dtype=torch.float64, device=w.device)
        b = torch.zeros(cout, dtype=torch.float64, device=w.device)
    else:
        s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        b = bn.bias.detach().double() - bn.running_mean.detach().double() * s
    w = w * s[:, None, None, None]
    cout_p = _cp(cout)
    if stem:                                            # im2col columns c * 9 + ky * 3 + kx, padded to 32
        wf = torch.zeros(cout_p, 32, dtype=torch.float64, device=w.device)
        wf[:cout, :27] = w.reshape(cout, 27)
    else:
        wf = torch.zeros(cout_p, k * k, cin_p, dtype=torch.float64, device=w.device)
        wf[:cout, :, :cin] = w.permute(0, 2, 3, 1).reshape(cout, k * k, cin)
        wf = wf.reshape(cout_p, k * k * cin_p)
    bf = torch.zeros(cout_p, dtype=torch.float64, device=w.device)
    bf[:cout] = b
    return wf.float().contiguous(), bf.float().contiguous()


class ModifiedResNet(nn.Module):
    """CLIP ResNet image encoder; `forward(frames [F,3,R,R]) -> [F, output_dim]` runs acx_resnet_encode in chunks of `chunk`
    frames in eval mode (workspace allocated once per chunk size and reused), acx_resnet_encode_train over all F frames in training
    mode (the BatchNorms' batch statistics span every frame of the call)."""

    def __init__(self, layers: Sequence[int], output_dim: int, heads: int, input_resolution: int = 224, width: int = 64,
                 precision: str = "auto", chunk: int = 512, arch: Optional[str] = None):
        super().__init__()
        self.arch = arch or f"ResNet(layers {tuple(layers)}, width {width}, resolution {input_resolution})"
        self.output_dim, self.input_resolution, self.width, self.heads = output_dim, input_resolution, width, heads
        self.layers_ = tuple(int(n) for n in layers)
        self.conv1 = nn.Conv2d(3, width // 2, kernel_size=3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(width // 2)
        self.conv2 = nn.Conv2d(width // 2, width // 2, kernel_size=3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(width // 2)
        self.conv3 = nn.Conv2d(width // 2, width, kernel_size=3, padding=1, bias=False)
        self.bn3 = nn.BatchNorm2d(width)
        self.avgpool = nn.AvgPool2d(2)
        self._inplanes = width
        self.layer1 = self._make_layer(width, layers[0])
        self.layer2 = self._make_layer(width * 2, layers[1], stride=2)
        self.layer3 = self._make_layer(width * 4, layers[2], stride=2)
        self.layer4 = self._make_layer(width * 8, layers[3], stride=2)
        self.attnpool = AttentionPool2d(input_resolution // 32, width * 32, heads, output_dim)
        self.precision = precision
        check_resnet_precision(precision, self.arch, width)
        self.chunk = chunk
        self._wcache = None
        self._tcache = None
        self._ws: Optional[torch.Tensor] = None

    def _make_layer(self, planes: int, blocks: int, stride: int = 1):
        layers = [Bottleneck(self._inplanes, planes, stride)]
        self._inplanes = planes * 4
        for _ in range(1, blocks):
            layers.append(Bottleneck(self._inplanes, planes))
        return nn.Sequential(*layers)

    def blocks(self) -> List[Bottleneck]:
        return [b for layer in (self.layer1, self.layer2, self.layer3, self.layer4) for b in layer]

    def desc(self) -> "L.ResnetDesc":
        return L.ResnetDesc(self.input_resolution, self.width, (C.c_int32 * 4)(*self.layers_), self.heads, self.output_dim,
                            RESNET_PRECISIONS[self.precision])

    def _weights(self, fold: bool = True):
        """The acx_resnet_weights table: BatchNorms folded (eval), or the raw convolution weights (training mode); cached by weight
        epoch and the address / version of every parameter and buffer.  precision "bf16x6" (eval): plus the three bf16 planes of
        every folded weight the driver routes to the plane kernel -- part of the same cache entry, which is keyed by the precision
        as well (a table built for one precision is never handed to another)."""
        x6 = fold and self.precision == "bf16x6"
        key = (ops.WEIGHT_EPOCH[0], x6) + tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))
        cache = self._wcache if fold else self._tcache
        if cache is not None and cache[0] == key:
            return cache[1]
        keep = []
        split = []                                  # (f32 weight, its [3, Cout_p, K] bf16 planes): one launch at the end
        w = L.ResnetWeights()

        def planes(wf):
            w3 = torch.empty((3,) + tuple(wf.shape), dtype=torch.bfloat16, device=wf.device)
            split.append((wf, w3))
            keep.append(w3)
            return w3.data_ptr()

        def put(dst, conv, bn, cin_p, stem=False):
            wf, bf = _fold(conv, bn if fold else None, cin_p, stem)
            keep.extend((wf, bf))
            dst.w, dst.b = wf.data_ptr(), bf.data_ptr()
            if x6 and not stem and _routed(wf.shape[1], conv.kernel_size[0] == 3):
                dst.w3 = planes(wf)
        put(w.stem[0], self.conv1, self.bn1, 32, stem=True)
        put(w.stem[1], self.conv2, self.bn2, _cp(self.width // 2))
        put(w.stem[2], self.conv3, self.bn3, _cp(self.width // 2))
        blocks = self.blocks()
        arr = (L.ResnetBlock * len(blocks))()
        for i, b in enumerate(blocks):
            cin_p = _cp(b.conv1.weight.shape[1])
            put(arr[i].conv1, b.conv1, b.bn1, cin_p)
            put(arr[i].conv2, b.conv2, b.bn2, _cp(b.conv2.weight.shape[1]))
            put(arr[i].conv3, b.conv3, b.bn3, _cp(b.conv3.weight.shape[1]))
            if b.downsample is not None:
                put(arr[i].downsample, b.downsample[1], b.downsample[2], cin_p)
        w.blocks = C.cast(arr, C.POINTER(L.ResnetBlock))
        ap = self.attnpool
        kv_w = torch.cat([ap.k_proj.weight.detach(), ap.v_proj.weight.detach()]).contiguous()
        kv_b = torch.cat([ap.k_proj.bias.detach(), ap.v_proj.bias.detach()]).contiguous()
        keep += [arr, kv_w, kv_b]
        w.positional_embedding = ap.positional_embedding.data_ptr()
        w.q_w, w.q_b = ap.q_proj.weight.data_ptr(), ap.q_proj.bias.data_ptr()
        w.kv_w, w.kv_b = kv_w.data_ptr(), kv_b.data_ptr()
        if x6 and _routed(kv_w.shape[1], False):
            w.kv_w3 = planes(kv_w)
        ops.split_bf16x3_multi(split)
        w.c_w, w.c_b = ap.c_proj.weight.data_ptr(), ap.c_proj.bias.data_ptr()
        if fold:
            self._wcache = (key, (w, keep))
        else:
            self._tcache = (key, (w, keep))
        return (w, keep)

    def _bn_table(self):
        """acx_resnet_train_bn: device pointers to every BatchNorm's parameters and buffers (updated in place by the call)."""
        def put(dst, bn):
            for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var):
                assert t.is_contiguous() and t.dtype == torch.float32
            dst.weight, dst.bias = bn.weight.data_ptr(), bn.bias.data_ptr()
            dst.running_mean, dst.running_var = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
            dst.num_batches_tracked = bn.num_batches_tracked.data_ptr() if bn.num_batches_tracked is not None else None
        t = L.ResnetTrainBn()
        for i, bn in enumerate((self.bn1, self.bn2, self.bn3)):
            put(t.stem[i], bn)
        blocks = self.blocks()
        arr = (L.ResnetBlockBn * len(blocks))()
        for i, b in enumerate(blocks):
            put(arr[i].bn1, b.bn1)
            put(arr[i].bn2, b.bn2)
            put(arr[i].bn3, b.bn3)
            if b.downsample is not None:
                put(arr[i].downsample, b.downsample[2])
        t.blocks = C.cast(arr, C.POINTER(L.ResnetBlockBn))
        t.eps, t.momentum = self.bn1.eps, self.bn1.momentum
        return t, arr

    def _forward_train(self, x: torch.Tensor) -> torch.Tensor:
        """BatchNorm2d in training mode over ALL frames of the call (one launch sequence; chunking would change the statistics)."""
        lib = L.lib()
        d = self.desc()
        w, _keep = self._weights(fold=False)
        bn, _arr = self._bn_table()
        F = x.shape[0]
        out = torch.empty(F, self.output_dim, dtype=torch.float32, device=x.device)
        nbytes = lib.acx_resnet_train_workspace_bytes(C.byref(d), F)
        if nbytes == 0:
            raise ValueError(f"{self.arch}: geometry not supported by acx_resnet_encode_train")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        h = ops._h(x)
        L.check(lib.acx_resnet_encode_train(h, C.byref(d), C.byref(w), C.byref(bn), x.data_ptr(), F, out.data_ptr(), ws.data_ptr(),
                                            nbytes, ops._stream()), h)
        # the running statistics changed in place (their _version did not): the folded eval weights are stale
        self._wcache = None
        return out

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        R = self.input_resolution
        assert x.dim() == 4 and x.shape[1] == 3 and x.shape[2] == x.shape[3] == R
        check_resnet_precision(self.precision, self.arch, self.width)
        x = x.contiguous().float()
        if self.training:
            return self._forward_train(x)
        lib = L.lib()
        d = self.desc()
        w, _keep = self._weights()
        F = x.shape[0]
        out = torch.empty(F, self.output_dim, dtype=torch.float32, device=x.device)
        chunk = min(self.chunk, F)
        nbytes = lib.acx_resnet_workspace_bytes(C.byref(d), chunk)
        if nbytes == 0:
            raise ValueError(f"{self.arch}: geometry not supported by acx_resnet_encode")
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != x.device:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        h = ops._h(x)
        s = ops._stream()
        for f0 in range(0, F, chunk):
            n = min(chunk, F - f0)
            L.check(lib.acx_resnet_encode(h, C.byref(d), C.byref(w), x[f0:f0 + n].data_ptr(), n, out[f0:f0 + n].data_ptr(),
                                          self._ws.data_ptr(), self._ws.numel(), s), h)
        return out
