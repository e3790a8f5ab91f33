"""Timing of the ViT attention kernels at 512 frames x 12 heads x 197 tokens (development probe; ACX_LIB_PATH selects an A/B build:
a library without acx_attention_p3f skips that arm).  The f32 input is 930 MB, the planes 1.39 GB: neither is served by the 256 MiB
Infinity Cache."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from anomalyclip_amd import ops, _lib as L
from bench import _event_time

dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(1)
B, L_, H = 512, 197, 12
qkv = torch.randn(B * L_, 3 * H * 64, generator=g, device=dev)
q3 = ops.split_bf16x3(qkv, panel=True)
fl = 4.0 * B * H * L_ * L_ * 64
t32 = _event_time(lambda: ops.attention(qkv, B, L_, H, False), 8)
tp3 = _event_time(lambda: ops.attention_p3(q3, B, L_, H), 8)
print(f"f32 MFMA attention {t32 * 1e3:.3f} ms {fl / t32 / 1e12:.1f} TFLOP/s | planes attention {tp3 * 1e3:.3f} ms "
      f"{fl / tp3 / 1e12:.1f} TF-equiv ({6 * fl / tp3 / 1e12:.0f} bf16 TF)")
try:
    same = torch.equal(ops.attention_p3_f32(qkv, B, L_, H).view(torch.int16), ops.attention_p3(q3, B, L_, H).view(torch.int16))
    tpf = _event_time(lambda: ops.attention_p3_f32(qkv, B, L_, H), 8)
    print(f"planes attention, f32 q|k|v in {tpf * 1e3:.3f} ms {fl / tpf / 1e12:.1f} TF-equiv ({6 * fl / tpf / 1e12:.0f} bf16 TF): "
          f"{(tp3 - tpf) * 1e3:+.3f} ms against planes in, outputs {'equal bit for bit' if same else 'DIFFERENT (an ablation build?)'}")
except L.AcxError as e:
    print("f32-input arm skipped:", e)
