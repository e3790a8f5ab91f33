"""`AnomalyCLIPDataModule` (the reference's src/data/anomaly_clip_datamodule.py), without Lightning: same hyper-parameter keys, same
loader methods, same batch tuples.

`load_from_features: true`: training batches come from a `FeatureBank` of the feature files, resident in device memory, through two
`ResidentTrainLoader`s (normal / abnormal videos, batch_size // 2 each: anomaly_clip_datamodule.py:144-163); the test-mode loaders
stream the files through `FeatureStream` and add the per-frame labels of the temporal annotation file (feature_dataset.py:329-345).

`load_from_features: false` with `encoder=`: the frame folders `<frames_root>/<video>/<image_tmpl>` are encoded ONCE by the frozen
CLIP image encoder into such banks (`FeatureBank.from_frames`; the reference's frame transform is deterministic, so its per-step
encoding gives the same rows) and every loader draws from a bank: `ResidentTrainLoader` as above, `ResidentTestLoader` for the
test-mode tiles.  No feature file is written.  `decode="gpu"` (a keyword beside `encoder=`, not one of the reference's keys) has the
frames' baseline JPEG files reconstructed on the device (anomalyclip_amd/jpeg.py) instead of decoded by Pillow, `decode="gpu_entropy"` their Huffman decoding too: the same banks.

`annotation_file_predict` (optional, not one of the reference's keys) lists videos WITHOUT ground truth, rows `path start_frame
end_frame [label]`; `predict_dataloader()` yields the test-mode tuples for them in both modes (Trainer.predict)."""
from __future__ import annotations

import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .anomaly_clip_module import AttrDict
from .feature_bank import BankTile, FeatureBank, ResidentTrainLoader
from .feature_stream import FeatureStream

HPARAM_KEYS = ("frames_root", "annotation_file_normal", "annotation_file_anomaly", "annotation_file_test",
               "annotation_file_temporal_test", "labels_file", "normal_id", "num_classes", "num_segments", "seg_length", "ncrops",
               "stride", "batch_size", "batch_size_test", "load_from_features", "visualize", "image_tmpl")
_DEFAULTS = dict(annotation_file_temporal_test=None, annotation_file_predict=None, labels_file=None, num_segments=32, seg_length=16, ncrops=1, stride=1,
                 batch_size=64, batch_size_test=1, load_from_features=True, visualize=False, image_tmpl="{:06d}.jpg")


class VideoRecord:
    """one annotation row `path start_frame end_frame label` (feature_dataset.py:42-95)"""

    def __init__(self, row: Sequence[str], root: str, where: str):
        if len(row) != 4:
            raise ValueError(f"{where}: expected `path start_frame end_frame label`, got {' '.join(row)!r}")
        self.video = row[0]                                      # the frame folder under frames_root
        self.path = os.path.join(root, row[0]) + ".npy"
        self.start_frame, self.end_frame, self.label = int(row[1]), int(row[2]), int(row[3])

    @property
    def num_frames(self) -> int:
        return self.end_frame - self.start_frame + 1            # the end frame is inclusive


def read_annotation_file(path: str, root: str) -> List[VideoRecord]:
    with open(path) as fh:
        return [VideoRecord(line.strip().split(), root, f"{path}:{i + 1}") for i, line in enumerate(fh) if line.strip()]


def read_predict_file(path: str, root: str, normal_id: int) -> List[VideoRecord]:
    """the list of unlabeled videos (`annotation_file_predict`): rows `path start_frame end_frame [label]`; the label column is
    optional and ignored (a row of one of the labeled lists can be used as it is): every record carries `normal_id`"""
    out = []
    with open(path) as fh:
        for i, line in enumerate(fh):
            row = line.strip().split()
            if not row:
                continue
            if len(row) not in (3, 4):
                raise ValueError(f"{path}:{i + 1}: expected `path start_frame end_frame [label]`, got {' '.join(row)!r}")
            out.append(VideoRecord(row[:3] + [str(int(normal_id))], root, f"{path}:{i + 1}"))
    return out


def read_temporal_annotations(path: Optional[str]) -> Dict[str, np.ndarray]:
    """{video stem: int64 [pairs, 2] of (start, stop)}: key = stem of the first column, values = the fields from the third on"""
    out: Dict[str, np.ndarray] = {}
    if path:
        with open(path) as fh:
            for line in fh:
                f = line.strip().split()
                if f:
                    v = np.asarray([int(x) for x in f[2:]], dtype=np.int64)
                    out[str(Path(f[0]).stem)] = v[: len(v) // 2 * 2].reshape(-1, 2)
    return out


def frame_labels(frames: int, start_frame: int, label: int, normal_id: int, pairs: np.ndarray) -> np.ndarray:
    """per-frame labels int64 [frames]: frame i carries `label` iff start <= i + start_frame <= stop for some (start, stop) pair,
    else `normal_id` (a `-1 -1` pair matches nothing)"""
    pos = np.arange(frames, dtype=np.int64) + start_frame
    hit = ((pairs[:, :1] <= pos[None, :]) & (pos[None, :] <= pairs[:, 1:])).any(0) if len(pairs) else np.zeros(frames, dtype=bool)
    return np.where(hit, np.int64(label), np.int64(normal_id))


class StreamedTestLoader:
    """The reference's test-mode dataset under DataLoader(batch_size=1, shuffle=False): yields
    (features [1, ncrops, rows, D] on the device, labels [1, T] int64, label [1], segment_size [1], [path]).  The tile is sized by
    the FILE's frame count (FeatureStream), which is the annotation row's in every list the reference ships."""

    def __init__(self, records: List[VideoRecord], annotations: Optional[Dict[str, np.ndarray]], hp, device):
        self.records, self.annotations, self.hp, self.device = records, annotations, hp, device

    def __len__(self) -> int:
        return len(self.records)

    def frame_labels(self, i: int, frames: int) -> np.ndarray:
        """per-frame labels int64 [frames] of record i, whose file holds `frames` frames"""
        rec, hp = self.records[i], self.hp
        pairs = np.zeros((0, 2), dtype=np.int64)
        if self.annotations:
            stem = Path(rec.path).stem
            if stem not in self.annotations:
                raise KeyError(f"{rec.path}: no row for {stem!r} in {hp.annotation_file_temporal_test}")
            pairs = self.annotations[stem]
        return frame_labels(frames, rec.start_frame, rec.label, int(hp.normal_id), pairs)

    def __iter__(self):
        hp = self.hp
        stream = FeatureStream([r.path for r in self.records], int(hp.num_segments), int(hp.seg_length), int(hp.stride),
                               int(hp.ncrops), device=self.device)
        for i, (feats, T, S, path) in enumerate(stream):
            lab = torch.from_numpy(self.frame_labels(i, T)).unsqueeze(0)
            yield feats, lab, torch.tensor([self.records[i].label]), torch.tensor([S]), [path]


class ResidentTestLoader(StreamedTestLoader):
    """The same 5-tuples over the first len(records) videos of a resident bank (`records[i]` is video i of `bank`: the normal list
    heads the training bank): the features are a `BankTile`,
    gathered on the device when the consumer asks (`.to(device)`, or a group at once in AnomalyCLIPModule.score_videos); `path`
    is the bank's path of the video (the frame folder of a bank filled from frames)."""

    def __init__(self, bank: FeatureBank, records: List[VideoRecord], annotations: Optional[Dict[str, np.ndarray]], hp):
        super().__init__(records, annotations, hp, bank.device)
        if len(records) > len(bank):
            raise ValueError(f"ResidentTestLoader: {len(records)} records over a bank of {len(bank)} videos")
        self.bank = bank

    def __iter__(self):
        hp, bank = self.hp, self.bank
        for i, rec in enumerate(self.records):
            tile = BankTile(bank, i, int(hp.num_segments), int(hp.seg_length), int(hp.stride))
            lab = torch.from_numpy(self.frame_labels(i, bank.file_frames[i])).unsqueeze(0)
            yield tile, lab, torch.tensor([rec.label]), torch.tensor([tile.S]), [bank.paths[i]]


class AnomalyCLIPDataModule:
    def __init__(self, encoder=None, decode: str = "pil", pack: bool = False, bank_dtype: str = "float32", **hparams):
        from .feature_bank import check_bank_dtype
        from .jpeg import check_decode
        check_bank_dtype(bank_dtype)
        self.bank_dtype = bank_dtype                              # frames mode: the banks' element type (not a reference key)
        self.pack = bool(pack)                                    # frames mode: FeatureBank.from_frames(pack=...) (not a reference key)
        self.decode = check_decode(decode)                        # frames mode: how the frame files are decoded (not a reference key)
        hp = dict(_DEFAULTS)
        hp.update(hparams)                                        # unknown keys are kept, like save_hyperparameters does
        missing = [k for k in HPARAM_KEYS if k not in hp]
        if missing:
            raise TypeError(f"AnomalyCLIPDataModule: missing hyper-parameters {missing}")
        if not hp["load_from_features"]:
            if encoder is None:
                raise ValueError("AnomalyCLIPDataModule: load_from_features=False (training from frame folders) needs the CLIP image "
                                 "encoder that turns the frames into features: pass encoder=<the AnomalyCLIP net or its "
                                 "image_encoder>, or extract feature files first (anomalyclip_amd.extract)")
            if int(hp["ncrops"]) not in (1, 5, 10):
                raise ValueError(f"AnomalyCLIPDataModule: ncrops={hp['ncrops']} with load_from_features=False: frames are cropped 1, 5 "
                                 f"or 10 times (anomalyclip_amd.extract)")
        self.encoder = None if hp["load_from_features"] else getattr(encoder, "image_encoder", encoder)
        if int(hp["batch_size_test"]) != 1:
            raise ValueError("AnomalyCLIPDataModule: batch_size_test must be 1 (videos differ in length)")
        self.hparams = AttrDict(hp)
        self.device: Optional[torch.device] = hp.get("device")
        self.bank: Optional[FeatureBank] = None
        self.normal: List[VideoRecord] = []
        self.anomaly: List[VideoRecord] = []
        self.test: List[VideoRecord] = []
        self._annotations: Dict[str, np.ndarray] = {}
        self._train_loaders = None
        self._test_bank: Optional[FeatureBank] = None             # frames mode: the test list's bank ...
        self._normal_bank: Optional[FeatureBank] = None           # ... and the normal list's, when no fit bank holds it
        self.predict: List[VideoRecord] = []                      # `annotation_file_predict`: videos without ground truth ...
        self._predict_bank: Optional[FeatureBank] = None          # ... and, frames mode, their bank

    @property
    def yields_features(self) -> bool:
        """every loader yields FEATURES, whatever `load_from_features` says (frames are encoded into banks here)"""
        return True

    @property
    def num_classes(self):
        return self.hparams.num_classes

    def prepare_data(self):
        pass

    def _read_lists(self):
        hp = self.hparams
        if not self.test and not self.normal:
            self.normal = read_annotation_file(hp.annotation_file_normal, hp.frames_root)
            self.anomaly = read_annotation_file(hp.annotation_file_anomaly, hp.frames_root)
            self.test = read_annotation_file(hp.annotation_file_test, hp.frames_root)
            self._annotations = read_temporal_annotations(hp.annotation_file_temporal_test)

    def _frames_bank(self, records: List[VideoRecord]) -> FeatureBank:
        """frames mode: the bank of `records`, encoded now.  The encoder is put in eval mode for the pass (BatchNorm on running
        statistics, as extraction demands) and left as it was."""
        hp, enc = self.hparams, self.encoder
        was_training = enc.training
        enc.eval()
        try:
            return FeatureBank.from_frames(enc, records, hp.frames_root, hp.image_tmpl, int(hp.ncrops), hp.get("scale_size"),
                                           int(hp.get("decode_threads", 8)), self.device, hp.get("max_bytes"), hp.get("log"),
                                           decode=self.decode, pack=self.pack, bank_dtype=self.bank_dtype)
        finally:
            enc.train(was_training)

    def setup(self, stage: Optional[str] = None):
        """reads the lists; for `fit` (or no stage) loads ONE bank over the normal and the abnormal training videos (frames mode:
        encodes it; the test list's bank is encoded when its loader is first asked for)"""
        self._read_lists()
        if stage in (None, "fit") and self.bank is None:
            hp = self.hparams
            recs = self.normal + self.anomaly
            if self.encoder is not None:
                self.bank = self._frames_bank(recs)
            else:
                self.bank = FeatureBank([r.path for r in recs], [r.num_frames for r in recs], [r.label for r in recs],
                                        ncrops=int(hp.ncrops), device=self.device, max_bytes=hp.get("max_bytes"))

    def train_dataloader(self):
        if self.bank is None:
            self.setup("fit")
        if self._train_loaders is None:           # kept across epochs: pinned slots, shard seed and epoch counter live in them
            hp, n = self.hparams, len(self.normal)
            kw = dict(batch_size=int(hp.batch_size) // 2, num_segments=int(hp.num_segments), seg_length=int(hp.seg_length),
                      stride=int(hp.stride), shuffle=True, drop_last=True)
            self._train_loaders = [ResidentTrainLoader(self.bank, range(n), **kw),
                                   ResidentTrainLoader(self.bank, range(n, n + len(self.anomaly)), **kw)]
        return self._train_loaders

    def val_dataloader(self):
        self._read_lists()
        if self.encoder is not None:
            if self._test_bank is None:
                self._test_bank = self._frames_bank(self.test)
            return ResidentTestLoader(self._test_bank, self.test, self._annotations, self.hparams)
        return StreamedTestLoader(self.test, self._annotations, self.hparams, self.device)

    def test_dataloader(self):
        return self.val_dataloader()

    def predict_dataloader(self):
        """the test-mode 5-tuples of the videos of `annotation_file_predict`, which need no annotation: the label tensor is
        `normal_id` repeated T times and only its length means anything"""
        hp = self.hparams
        if not hp.get("annotation_file_predict"):
            raise ValueError("AnomalyCLIPDataModule.predict_dataloader: the hyper-parameter `annotation_file_predict` (rows `path "
                             "start_frame end_frame [label]`) is not set")
        if not self.predict:
            self.predict = read_predict_file(hp.annotation_file_predict, hp.frames_root, int(hp.normal_id))
        if self.encoder is not None:
            if self._predict_bank is None:
                self._predict_bank = self._frames_bank(self.predict)
            return ResidentTestLoader(self._predict_bank, self.predict, None, hp)
        return StreamedTestLoader(self.predict, None, hp, self.device)

    def train_dataloader_test_mode(self):
        self._read_lists()
        if self.encoder is not None:
            bank = self.bank                      # the fit bank's first len(normal) videos ARE the normal list
            if bank is None:
                if self._normal_bank is None:
                    self._normal_bank = self._frames_bank(self.normal)
                bank = self._normal_bank
            return ResidentTestLoader(bank, self.normal, None, self.hparams)
        return StreamedTestLoader(self.normal, None, self.hparams, self.device)       # (no temporal file: every frame normal_id)

    def resident_normal_videos(self):
        """the normal training videos' rows in the bank, in file order -- what `train_dataloader_test_mode()` would stream again
        -- when a frame is one bank row and the test-mode tile keeps the file's order (one crop, stride 1); else None"""
        if self.bank is None or int(self.hparams.ncrops) != 1 or int(self.hparams.stride) != 1:
            return None
        return [self.bank.video(v) for v in range(len(self.normal))]

    def teardown(self, stage: Optional[str] = None):
        pass

    def state_dict(self):
        return {}

    def load_state_dict(self, state_dict):
        pass
