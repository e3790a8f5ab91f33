"""Generates tests/golden/train_batches.npz by EXECUTING THE REFERENCE's train-mode feature dataset.

Run in the development container only (needs the reference checkout, see ref_harness.py):
    python tests/golden/make_golden_train.py

Per case of recipes_train.CASES: the recipe's files -> the reference's VideoFrameDataset (train mode) under
torch.utils.data.DataLoader(shuffle=True, drop_last=True, batch_size=2), two epochs after torch.manual_seed(3);
np.random.seed(5).  Stored per batch k of a case X: `X_feat{k}` (the batch), `X_label{k}`, and what the dataset drew for it,
recorded while it ran: `X_vid{k}` (the sampler's video indices) and `X_starts{k}` (the start indices of each video).  The error
case is run too: the reference must raise ValueError on it.  What is captured is DATA; no reference source is stored."""
import importlib
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_harness as H  # noqa: E402
import recipes_train as RT  # noqa: E402

H.install()
fd = importlib.import_module("src.data.components.feature_dataset")


def dataset(directory, ann, case):
    return fd.VideoFrameDataset(root_path=str(directory), annotationfile_path=ann, normal_id=0, num_segments=case["N"],
                                frames_per_segment=case["L"], test_mode=False, ncrops=case["ncrops"], stride=case["stride"])


def run_case(name, case, arrs):
    with tempfile.TemporaryDirectory() as d:
        ann, paths, frames, labels = RT.write_case(d, case)
        ds = dataset(d, ann, case)
        drawn = []                                   # (video index, start indices) in the order the dataset was asked
        inner = ds._get_start_indices

        def spy(record):
            s = inner(record)
            drawn.append((ds.video_list.index(record), np.asarray(s, dtype=np.int64)))
            return s
        ds._get_start_indices = spy
        torch.manual_seed(RT.TORCH_SEED)
        np.random.seed(RT.NUMPY_SEED)
        loader = torch.utils.data.DataLoader(ds, shuffle=True, drop_last=True, batch_size=RT.BATCH)
        k = 0
        for _ in range(RT.EPOCHS):
            for feats, label in loader:
                mine, drawn[:] = drawn[:RT.BATCH], drawn[RT.BATCH:]
                assert len(mine) == RT.BATCH and feats.shape == (RT.BATCH, case["ncrops"], case["N"] * case["L"], RT.D)
                arrs[f"{name}_feat{k}"] = feats.numpy().astype(np.float32)
                arrs[f"{name}_label{k}"] = label.numpy().astype(np.int64)
                arrs[f"{name}_vid{k}"] = np.asarray([v for v, _ in mine], dtype=np.int64)
                arrs[f"{name}_starts{k}"] = np.stack([s for _, s in mine])
                assert [labels[v] for v, _ in mine] == label.tolist()
                k += 1
        arrs[f"{name}_batches"] = k
        print(f"case {name}: {k} batches")


def run_error_case(arrs):
    with tempfile.TemporaryDirectory() as d:
        ann, *_ = RT.write_case(d, RT.ERROR_CASE)
        ds = dataset(d, ann, RT.ERROR_CASE)
        raised = []
        for i in range(len(ds)):
            try:
                ds[i]
                raised.append(0)
            except ValueError:
                raised.append(1)
        assert raised[0] == 1, raised
        arrs["error_raised"] = np.asarray(raised, dtype=np.int64)
        print("error case: ValueError per video", raised)


if __name__ == "__main__":
    arrs = {}
    for name, case in RT.CASES.items():
        run_case(name, case, arrs)
    run_error_case(arrs)
    path = os.path.join(HERE, "train_batches.npz")
    np.savez_compressed(path, **arrs)
    print(f"train_batches.npz  {os.path.getsize(path) / 1024:.1f} KiB")
