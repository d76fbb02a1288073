"""Device-resident MNIST training set with a stateless batch sequence.

The whole training set stays on the device as uint8 (47 MB for 60000
images); a batch is built by ONE gather (ops/functional.py::batch_gather —
the HIP batch_gather_kernel for bf16 on a GPU, the torch reference
elsewhere) that permutes, normalises through a 256-entry LUT and writes
straight into the caller's buffers.  No host array is touched per step.

The sample order is a pure function of (seed, step): epoch = step // spe
with spe = N // B batches per epoch (the N % B tail is dropped, as
DataSet.next_batch drops it), epoch 0 unshuffled (as DataSet), later epochs
ordered by a cycle-walking Feistel permutation keyed on (seed, epoch) —
ops/cpu_ref.py::feistel_perm.  A resumed run that seeks to its restored step
therefore sees exactly the batches an uninterrupted run would have seen.

Optional affine augmentation (small random shifts / rotations / scalings)
runs inside the same gather: a table of T integer inverse-affine maps is
built once from the data set's seed (ops/cpu_ref.py::augment_table) and
lives on the device; batch position j at `step` is warped by table row
aug_indices(seed, step, j), again a pure function of (seed, step), so resume
and hipGraph capture keep working unchanged.  Evaluation (range_into) never
augments.
"""

from __future__ import annotations

import os

import numpy as np
import torch

from ..ops import functional as Fx
from ..ops.cpu_ref import augment_table
from .mnist_data import (IMAGE_SIZE, NUM_CHANNELS, PIXEL_DEPTH, TEST_IMAGES,
                         TEST_LABELS, TRAIN_IMAGES, TRAIN_LABELS,
                         extract_images_u8, extract_labels)


def normalisation_lut(dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """lut[v] = (v - 127.5) / 255 — extract_images' normalisation, evaluated
    in fp32 and rounded once to `dtype` (the same rounding the host-fed path
    applies when it casts its fp32 batch)."""
    lut = (torch.arange(256).float() - PIXEL_DEPTH / 2.0) / PIXEL_DEPTH
    return lut.to(dtype)


class DeviceDataSet:
    """Drop-in for DataSet whose data lives on `device` as uint8.

    images_u8: [N, 784] (or [N,28,28[,1]]) uint8; labels: [N] integer < 256.
    Sharding follows DataSet: rank::world slices unless shard=False.

    Augmentation: any of augment_shift (px) / augment_rotate (deg) /
    augment_scale (frac) above 0 builds a table of augment_table_size
    transforms from `seed`; a ready int32 [T,6] `aug_table` takes precedence.
    """

    def __init__(self, images_u8, labels_u8, worker_id: int = 0,
                 n_workers: int = 1, shard: bool = True, seed: int = 0,
                 device="cpu", dtype: torch.dtype = torch.float32,
                 augment_shift: float = 0.0, augment_rotate: float = 0.0,
                 augment_scale: float = 0.0, augment_table_size: int = 4096,
                 aug_table=None):
        images_u8 = np.asarray(images_u8)
        labels_u8 = np.asarray(labels_u8)
        if images_u8.dtype != np.uint8:
            raise TypeError("DeviceDataSet wants raw uint8 pixels")
        assert images_u8.shape[0] == labels_u8.shape[0]
        images_u8 = images_u8.reshape(images_u8.shape[0], -1)
        assert images_u8.shape[1] == IMAGE_SIZE * IMAGE_SIZE * NUM_CHANNELS
        if shard and n_workers > 1:
            images_u8 = images_u8[worker_id::n_workers]
            labels_u8 = labels_u8[worker_id::n_workers]
        self._num_examples = int(images_u8.shape[0])
        self.device = torch.device(device)
        self.dtype = dtype
        self.seed = int(seed)
        # one private contiguous copy (the loader's arrays are read-only
        # views of the file buffer, shards are strided views)
        self._images = torch.from_numpy(np.array(images_u8)).to(self.device)
        self._labels = torch.from_numpy(
            np.array(labels_u8, dtype=np.uint8)).to(self.device)
        self._lut = normalisation_lut(dtype).to(self.device)
        self._cursor = 0
        if aug_table is None and max(augment_shift, augment_rotate,
                                     augment_scale) > 0:
            aug_table = augment_table(augment_table_size, self.seed,
                                      augment_shift, augment_rotate,
                                      augment_scale)
        self._aug_table = None
        if aug_table is not None:
            tab = torch.as_tensor(np.asarray(aug_table))
            if tab.dtype != torch.int32 or tab.dim() != 2 \
                    or tab.shape[1] != 6 or tab.shape[0] < 1:
                raise ValueError("aug_table must be int32 [T >= 1, 6]")
            self._aug_table = tab.contiguous().to(self.device)

    @property
    def aug_table(self):
        """int32 [T,6] on the device, or None when augmentation is off."""
        return self._aug_table

    @property
    def images(self):
        return self._images

    @property
    def labels(self):
        return self._labels

    @property
    def num_examples(self):
        return self._num_examples

    @property
    def epochs_completed(self):
        return None  # depends on the batch size: steps // (N // B)

    # -- stateless access ------------------------------------------------
    def gather_into(self, x: torch.Tensor, y: torch.Tensor, step=None,
                    step_dev=None, augment: bool = True):
        """Write the batch at `step` (host int) or `*step_dev` (device
        int64; capturable into a hipGraph) into x [B,28,28,1] / y [B],
        augmented when the data set has a table (augment=False: raw)."""
        if x.dtype != self.dtype:
            raise TypeError(f"x is {x.dtype}, data set built for {self.dtype}")
        return Fx.batch_gather(self._images, self._labels, self._lut, x, y,
                               self.seed, step=step, step_dev=step_dev,
                               aug_table=self._aug_table if augment else None)

    def range_into(self, x: torch.Tensor, y: torch.Tensor, start=None,
                   start_dev=None):
        """Write the sequential chunk [start, start + B) into x [B,28,28,1]
        / y [B]; `start` is a host int or `*start_dev` (device int64;
        capturable into a hipGraph).  Rows past the end of the set are
        zero-filled with label -1: evaluation reads the whole set, tail
        included, in fixed-shape chunks."""
        if x.dtype != self.dtype:
            raise TypeError(f"x is {x.dtype}, data set built for {self.dtype}")
        return Fx.range_gather(self._images, self._labels, self._lut, x, y,
                               start=start, start_dev=start_dev)

    @classmethod
    def random(cls, n: int, seed: int, device="cpu",
               dtype: torch.dtype = torch.float32, worker_id: int = 0,
               n_workers: int = 1, **augment):
        """Seeded uint8 stand-in (uniform pixels, labels in [0, 10)) for
        runs without idx-gz files."""
        rng = np.random.RandomState(seed)
        img = rng.randint(0, 256, size=(n, IMAGE_SIZE * IMAGE_SIZE),
                          dtype=np.uint8)
        lab = rng.randint(0, 10, size=n, dtype=np.uint8)
        return cls(img, lab, worker_id=worker_id, n_workers=n_workers,
                   seed=seed, device=device, dtype=dtype, **augment)

    def batch_at(self, step: int, batch_size: int, augment: bool = True):
        """(x, y) of the batch at `step` — a pure function of its arguments
        (and the seed).  augment=False gives the raw batch of an augmented
        data set."""
        if batch_size > self._num_examples:
            raise ValueError(f"batch size {batch_size} exceeds the "
                             f"{self._num_examples} examples of this rank")
        x = torch.empty((batch_size, IMAGE_SIZE, IMAGE_SIZE, NUM_CHANNELS),
                        dtype=self.dtype, device=self.device)
        y = torch.empty(batch_size, dtype=torch.int64, device=self.device)
        return self.gather_into(x, y, step=int(step), augment=augment)

    # -- DataSet-style cursor ---------------------------------------------
    def seek(self, step: int):
        self._cursor = int(step)

    def next_batch(self, batch_size: int):
        out = self.batch_at(self._cursor, batch_size)
        self._cursor += 1
        return out


def load_device_mnist(data_dir: str, subset: int = 0, worker_id: int = 0,
                      n_workers: int = 1, shard: bool = True, seed: int = 0,
                      device="cpu", dtype: torch.dtype = torch.float32,
                      split: str = "train", **augment):
    """idx-gz train files -> DeviceDataSet holding exactly the examples the
    host-fed path (engine/train.py::make_dataset) trains on: the rank::world
    shard unless shard=False, then `subset` keeps its first N examples.
    split="test" reads the t10k pair instead, same shard/subset rules.
    **augment: DeviceDataSet's augmentation arguments, passed through."""
    if split not in ("train", "test"):
        raise ValueError(f"split must be 'train' or 'test', not {split!r}")
    names = ((TRAIN_IMAGES, TRAIN_LABELS) if split == "train"
             else (TEST_IMAGES, TEST_LABELS))
    paths = [os.path.join(data_dir, f) for f in names]
    missing = [p for p in paths if not os.path.exists(p)]
    if missing:
        raise FileNotFoundError(
            f"MNIST files missing under {data_dir}: {missing}. This "
            "environment has no network; place the idx-gz files there or use "
            "--subset/fake data / synthetic mode.")
    images = extract_images_u8(paths[0])
    labels = extract_labels(paths[1])
    if shard and n_workers > 1:
        images, labels = images[worker_id::n_workers], labels[worker_id::n_workers]
    if subset:
        images, labels = images[:subset], labels[:subset]
    return DeviceDataSet(images, labels, shard=False, seed=seed,
                         device=device, dtype=dtype, **augment)
