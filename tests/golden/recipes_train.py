"""File recipes of tests/golden/train_batches.npz, shared by make_golden_train.py (which feeds the files to the REFERENCE's
train-mode dataset) and by the tests (which feed them to the resident loader).  File contents are arithmetic, so nothing but
the reference's batches is stored.  Pure numpy; no reference import."""
import os

import numpy as np

D = 8
TORCH_SEED, NUMPY_SEED = 3, 5          # torch.manual_seed / np.random.seed set before each case's loader is built
BATCH, EPOCHS = 2, 2

# name -> num_segments N, frames_per_segment L, stride, ncrops, file lengths T; `claims`: {video: frames the annotation row claims
# beyond the file's}.  Case E is case A with one such row: the draw is sized by the annotation, the wrap-around by the file.
CASES = {
    "A": dict(N=4, L=3, stride=1, ncrops=1, T=(1, 5, 12, 13, 40)),
    "B": dict(N=4, L=3, stride=2, ncrops=1, T=(1, 5, 12, 13, 40, 100)),
    "C": dict(N=4, L=3, stride=1, ncrops=2, T=(2, 7, 30)),
    "D": dict(N=32, L=16, stride=1, ncrops=1, T=(700, 100, 511, 513)),
    "E": dict(N=4, L=3, stride=1, ncrops=1, T=(1, 5, 12, 13, 40), claims={4: 9}),
}
ERROR_CASE = dict(N=2, L=16, stride=1, ncrops=1, T=(5, 33, 200))


def video_label(i: int) -> int:
    return (3 * i + 1) % 7


def write_case(directory, case: dict):
    """the case's feature files (video i: arange(T * ncrops * D).reshape(T * ncrops, D) + 1000 * i, float32) and its annotation
    file (`name 0 end label`) -> (annotation file, paths, num_frames per annotation row, labels)"""
    directory = str(directory)
    claims = case.get("claims", {})
    paths, frames, labels = [], [], []
    ann = os.path.join(directory, "train.txt")
    with open(ann, "w") as fa:
        for i, T in enumerate(case["T"]):
            rows = T * case["ncrops"]
            a = (np.arange(rows * D, dtype=np.float32).reshape(rows, D) + np.float32(1000 * i))
            name = f"v{i:02d}_{T}"
            np.save(os.path.join(directory, name + ".npy"), a)
            n = T + claims.get(i, 0)
            fa.write(f"{name} 0 {n - 1} {video_label(i)}\n")
            paths.append(os.path.join(directory, name + ".npy"))
            frames.append(n)
            labels.append(video_label(i))
    return ann, paths, frames, labels

