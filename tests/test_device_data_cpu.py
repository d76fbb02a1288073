"""Device-resident input pipeline, CPU side: the stateless epoch
permutation, DeviceDataSet through the torch reference, sharding/--subset,
and the trainer integration (trajectory equality with the host-fed path in
the first epoch; bit-identical resume)."""

import numpy as np
import pytest
import torch

from distributedmnist_amd.data import DeviceDataSet
from distributedmnist_amd.data.device_data import normalisation_lut
from distributedmnist_amd.data.mnist_data import write_random_idx
from distributedmnist_amd.ops.cpu_ref import batch_indices, feistel_perm

SEED = 66478


# -- perm ------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 37, 64, 65, 1000])
@pytest.mark.parametrize("epoch", [1, 2, 7])
def test_perm_is_a_bijection(n, epoch):
    out = feistel_perm(n, SEED, epoch, np.arange(n))
    assert sorted(out.tolist()) == list(range(n))


def test_perm_epoch0_is_identity():
    for n in (1, 37, 1000):
        assert feistel_perm(n, SEED, 0, np.arange(n)).tolist() == list(range(n))


def test_perm_golden_vectors():
    """Spec anchors: the kernel and this reference may not drift."""
    p = np.arange(5)
    assert feistel_perm(1000, SEED, 1, p).tolist() == [599, 994, 245, 23, 763]
    assert feistel_perm(60000, SEED, 2, p).tolist() == \
        [53611, 39760, 28312, 48359, 59041]
    assert feistel_perm(37, SEED, 1, p).tolist() == [25, 21, 4, 7, 33]


def test_perm_depends_on_epoch_and_seed():
    p = np.arange(1000)
    a = feistel_perm(1000, SEED, 1, p)
    assert not np.array_equal(a, feistel_perm(1000, SEED, 2, p))
    assert not np.array_equal(a, feistel_perm(1000, SEED + 1, 1, p))
    # the high seed word is part of the key
    assert not np.array_equal(a, feistel_perm(1000, SEED + (1 << 32), 1, p))


# -- DeviceDataSet on CPU ----------------------------------------------------

N, B = 37, 5
SPE = N // B  # 7 batches per epoch, 2 samples dropped


@pytest.fixture(scope="module")
def raw():
    rng = np.random.RandomState(3)
    img = rng.randint(0, 256, size=(N, 784), dtype=np.uint8)
    img[0, :256] = np.arange(256)  # every LUT entry is exercised
    lab = rng.randint(0, 10, size=N, dtype=np.uint8)
    return img, lab


def expect(img, lab, idx):
    lut = (np.arange(256, dtype=np.float32) - np.float32(127.5)) \
        / np.float32(255)
    return lut[img[idx]].reshape(-1, 28, 28, 1), lab[idx].astype(np.int64)


def test_batch_at_matches_lut_of_permuted_rows(raw):
    img, lab = raw
    ds = DeviceDataSet(img, lab, seed=SEED)
    assert ds.num_examples == N
    for s in range(2 * SPE + 3):  # across two epoch boundaries
        x, y = ds.batch_at(s, B)
        idx = batch_indices(N, B, SEED, s)
        ex, ey = expect(img, lab, idx)
        assert x.dtype == torch.float32 and x.shape == (B, 28, 28, 1)
        assert y.dtype == torch.int64
        assert np.array_equal(x.numpy(), ex), s
        assert np.array_equal(y.numpy(), ey), s
        if s < SPE:  # first epoch unshuffled, as DataSet
            assert idx.tolist() == list(range(s * B, s * B + B))


def test_each_epoch_holds_distinct_samples():
    for epoch in range(3):
        seen = np.concatenate([batch_indices(N, B, SEED, epoch * SPE + k)
                               for k in range(SPE)])
        assert len(set(seen.tolist())) == SPE * B == 35


def test_batch_equal_to_n_and_larger(raw):
    img, lab = raw
    ds = DeviceDataSet(img, lab, seed=SEED)
    for s in (0, 1, 5):
        x, y = ds.batch_at(s, N)
        idx = batch_indices(N, N, SEED, s)
        assert sorted(idx.tolist()) == list(range(N))
        assert np.array_equal(y.numpy(), lab[idx].astype(np.int64))
    with pytest.raises(ValueError):
        ds.batch_at(0, N + 1)
    with pytest.raises(ValueError):
        batch_indices(N, N + 1, SEED, 0)


def test_next_batch_after_seek_equals_batch_at(raw):
    img, lab = raw
    ds = DeviceDataSet(img, lab, seed=SEED)
    ds.seek(9)
    for s in (9, 10, 11):
        x, y = ds.next_batch(B)
        ex, ey = ds.batch_at(s, B)
        assert torch.equal(x, ex) and torch.equal(y, ey)


def test_huge_step_does_not_overflow(raw):
    img, lab = raw
    ds = DeviceDataSet(img, lab, seed=SEED)
    s = 10 ** 12
    epoch, pos = divmod(s, SPE)
    idx = feistel_perm(N, SEED, epoch, pos * B + np.arange(B))
    assert np.array_equal(batch_indices(N, B, SEED, s), idx)
    # the epoch enters the key schedule mod 2^32
    assert np.array_equal(idx, feistel_perm(N, SEED, epoch % 2 ** 32,
                                            pos * B + np.arange(B)))
    x, y = ds.batch_at(s, B)
    ex, ey = expect(img, lab, idx)
    assert np.array_equal(x.numpy(), ex) and np.array_equal(y.numpy(), ey)


def test_bf16_lut_is_the_rounded_fp32_normalisation(raw):
    img, lab = raw
    ds = DeviceDataSet(img, lab, seed=SEED, dtype=torch.bfloat16)
    x, _ = ds.batch_at(0, B)
    ex, _ = expect(img, lab, np.arange(B))
    assert x.dtype == torch.bfloat16
    assert torch.equal(x, torch.from_numpy(ex).to(torch.bfloat16))
    assert torch.equal(normalisation_lut(torch.bfloat16),
                       normalisation_lut().to(torch.bfloat16))


# -- sharding and --subset -----------------------------------------------------

def test_rank_world_sharding_odd_n(raw):
    img, lab = raw  # N = 37 is odd
    shards = [DeviceDataSet(img, lab, worker_id=r, n_workers=2, seed=SEED)
              for r in range(2)]
    assert [s.num_examples for s in shards] == [19, 18]
    for r, s in enumerate(shards):
        assert np.array_equal(s.images.numpy(), img[r::2])
        assert np.array_equal(s.labels.numpy(), lab[r::2])
    full = DeviceDataSet(img, lab, worker_id=1, n_workers=2, shard=False)
    assert full.num_examples == N


def _flags(tmp_path, *extra):
    from distributedmnist_amd.utils.flags import build_train_parser
    return build_train_parser().parse_args(
        ["--data_dir", str(tmp_path / "data"),
         "--train_dir", str(tmp_path / "td"), "--device", "cpu",
         "--save_interval_secs", "100000", *extra])


def test_make_dataset_subset_and_shard(tmp_path):
    from distributedmnist_amd.data.mnist_data import (extract_images_u8,
                                                      extract_labels)
    from distributedmnist_amd.engine.train import make_dataset
    write_random_idx(str(tmp_path / "data"), 64, 8, seed=1)
    img = extract_images_u8(str(tmp_path / "data" /
                                "train-images-idx3-ubyte.gz"))
    lab = extract_labels(str(tmp_path / "data" /
                             "train-labels-idx1-ubyte.gz"))
    cpu = torch.device("cpu")
    f = _flags(tmp_path, "--device_data", "--subset", "20", "--no_shard")
    ds = make_dataset(f, 1, 2, cpu, torch.float32)
    assert isinstance(ds, DeviceDataSet) and ds.num_examples == 20
    assert np.array_equal(ds.images.numpy(), img[:20])
    assert np.array_equal(ds.labels.numpy(), lab[:20].astype(np.uint8))
    # sharded: the same examples the host-fed DataSet of that rank holds
    f = _flags(tmp_path, "--device_data")
    ds = make_dataset(f, 1, 2, cpu, torch.float32)
    host = make_dataset(_flags(tmp_path), 1, 2, cpu, torch.float32)
    assert ds.num_examples == host.num_examples == 32
    assert np.array_equal(ds.images.numpy(), img[1::2])
    x, y = ds.batch_at(0, 32)
    assert np.array_equal(x.numpy(), host.images)
    assert np.array_equal(y.numpy(), host.labels)


def test_device_data_flag_ignored_for_synthetic(tmp_path, caplog):
    from distributedmnist_amd.data import SyntheticDataSet
    from distributedmnist_amd.engine.train import make_dataset
    f = _flags(tmp_path, "--device_data", "--synthetic_data")
    with caplog.at_level("INFO", logger="dmnist.train"):
        ds = make_dataset(f, 0, 1, torch.device("cpu"), torch.float32)
    assert isinstance(ds, SyntheticDataSet)
    assert "--device_data has no effect" in caplog.text


# -- trainer integration (CPU fp32 MLP, generated idx-gz, N=256) ---------------

def _train(tmp_path, tag, max_steps, *extra):
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    flags = _flags(tmp_path, "--model", "mlp", "--batch_size", "64",
                   "--train_dir", str(tmp_path / tag), *extra)
    t = Trainer(flags)
    ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
    hist = t.train(ds, max_steps=max_steps)
    return [h[3] for h in hist], t.fp.flat_master.clone(), t


def test_first_epoch_trajectory_equals_host_path(tmp_path):
    """Epoch 0 is unshuffled in both paths and both normalise with the
    same fp32 formula: the losses must be identical, not merely close."""
    write_random_idx(str(tmp_path / "data"), 256, 16, seed=2)
    spe = 256 // 64
    host, w_host, _ = _train(tmp_path, "host", spe)
    dev, w_dev, t = _train(tmp_path, "dev", spe, "--device_data")
    assert t._resident_ds is not None and len(dev) == spe
    assert host == dev
    assert torch.equal(w_host, w_dev)


def test_resume_sees_the_same_batches(tmp_path):
    """Straight to step 6 == checkpoint at 3, fresh Trainer, resume to 6
    (steps 4 and 5 lie in the shuffled second epoch).  The host DataSet
    cannot do this: its shuffle state is not checkpointed."""
    write_random_idx(str(tmp_path / "data"), 256, 16, seed=2)
    _, w_straight, _ = _train(tmp_path, "straight", 6, "--device_data")
    _, _, t3 = _train(tmp_path, "resumed", 3, "--device_data")
    assert t3.step == 3
    losses, w_resumed, t6 = _train(tmp_path, "resumed", 6, "--device_data")
    assert t6.step == 6 and len(losses) == 3  # restored at 3, ran 3 more
    assert torch.equal(w_straight, w_resumed)
