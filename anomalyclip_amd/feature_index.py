"""Test-mode frame/feature index logic of the reference's datasets:
`_get_start_indices` (feature_dataset.py:243-259) and the frame loop of `_get` (:359-367), vectorised
(one numpy gather instead of 512*S Python-level tensor indexings).  Bit-exact index tables are pinned by
tests/golden/tables.npz, which were produced by the reference's own code."""
from __future__ import annotations

import math

import numpy as np


def test_start_indices(num_frames: int, num_segments: int, frames_per_segment: int, stride: int = 1):
    """-> (start_indices int64 [num_segments*S], segment_size S)."""
    unit = num_segments * frames_per_segment * stride
    end_frame = math.ceil(num_frames / unit) * unit                       # round_to_nearest, feature_dataset.py:17-26
    starts = np.arange(end_frame / (frames_per_segment * stride)) * (frames_per_segment * stride)
    return starts.astype(np.int64), len(starts) // num_segments


def train_draw_range(num_frames: int, num_segments: int, frames_per_segment: int, stride: int = 1):
    """-> (distance between segment starts, exclusive upper bound of the random offset) of a train-mode draw
    (feature_dataset.py:260-276); a bound <= 0 is the video / grid pair the reference cannot sample."""
    lower = num_segments * frames_per_segment * stride
    span = num_frames if num_frames >= lower else lower
    dist = (span - frames_per_segment + 1) // num_segments
    return dist, dist + 2 - frames_per_segment


def train_start_indices(num_frames: int, num_segments: int, frames_per_segment: int, stride: int = 1, rng=None) -> np.ndarray:
    """Train-mode segment starts [num_segments] int64: evenly spaced segment origins plus ONE `rng.randint` call of
    num_segments offsets per video -- the reference's draw order is the contract.  `num_frames` is the annotation row's
    end - start + 1 (not the file's row count, which is what the frame index later wraps around).  `rng`: anything with
    numpy's `randint(high, size=)`, by default the global `np.random` like the reference."""
    dist, high = train_draw_range(num_frames, num_segments, frames_per_segment, stride)
    if high <= 0:
        raise ValueError(f"cannot draw train-mode starts for {num_frames} frames on a {num_segments} x {frames_per_segment} grid "
                         f"(stride {stride}): offset range {high} <= 0")
    rng = np.random if rng is None else rng
    return np.arange(num_segments, dtype=np.int64) * dist + rng.randint(high, size=num_segments)


def frame_index_table(start_indices: np.ndarray, frames_per_segment: int, stride: int, num_frames: int) -> np.ndarray:
    """flat list of source frame indices, wrapped modulo the video length (feature_dataset.py:362)."""
    off = np.arange(frames_per_segment, dtype=np.int64) * stride
    return ((start_indices[:, None].astype(np.int64) + off[None, :]) % num_frames).reshape(-1)


def gather_test_features(features: np.ndarray, num_segments: int, frames_per_segment: int, stride: int, ncrops: int = 1):
    """features [T*ncrops, D] (as stored in the .npy files) -> ([ncrops, N*S*L, D], segment_size), the tensor the
    reference's test loader yields (feature_dataset.py:347-376)."""
    D = features.shape[-1]
    f = features.reshape(-1, ncrops, D)                                   # (t, ncrops, D)
    T = f.shape[0]
    starts, S = test_start_indices(T, num_segments, frames_per_segment, stride)
    idx = frame_index_table(starts, frames_per_segment, stride, T)
    return np.ascontiguousarray(f[idx].transpose(1, 0, 2)), S
