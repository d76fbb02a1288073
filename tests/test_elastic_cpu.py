"""Elastic distortion, the integer definition (ops/cpu_ref.py): the smoothed
field against a float64 field, range and identity, purity, argument errors."""

import numpy as np
import pytest
import torch

from distributedmnist_amd.data import DeviceDataSet
from distributedmnist_amd.data.mnist_data import write_random_idx
from distributedmnist_amd.ops import cpu_ref
from distributedmnist_amd.ops.cpu_ref import (
    affine_warp_u8, augment_table, elastic_displacement, elastic_field,
    elastic_key, elastic_noise, elastic_taps, elastic_warp_u8)

SEED = 66478


def _float_gaussian(sigma):
    R = min(27, int(np.ceil(3.0 * sigma)))
    d = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-d * d / (2.0 * sigma * sigma))
    return R, w[R:] / w.sum()


@pytest.mark.parametrize("sigma", [1.0, 4.0, 16.0])
@pytest.mark.parametrize("step,j", [(0, 0), (7, 63), (10 ** 12, 1000)])
def test_integer_field_against_float64_field(sigma, step, j):
    """|F / 32768 - F64| <= 2 e1 + S / 65536, F64 = G64 . (N / 128) . G64^T.

    Derivation.  Write n = N / 128 (|n| <= 1), Gi = G / 256 (the integer
    taps as fractions), E = Gi - G64 and e1 = sum_d |g[|d|] / 256 - w(d) / Z|
    over -R..R: the largest absolute row sum of E, i.e. the tap rounding
    including the g[0] adjustment (worst case (2R + 1.5) / 256: half a unit
    per tap, plus at most R + 1 decrements of g[0]).  The first pass gives
    T8 = T / 256 + rho with |rho| <= 1/2, so

      F / 32768 = (Gi n + rho / 128) Gi^T
      F / 32768 - F64 = E n Gi^T + G64 n E^T + (rho / 128) Gi^T.

    Row sums of Gi are at most S / 256 <= 1 (S = g[0] + 2 sum g[d >= 1]) and
    of G64 at most 1, so the first two terms are at most e1 each and the
    third, half a T8 unit times the tap sum, at most (1 / 256)(S / 256)."""
    g = elastic_taps(sigma).astype(np.int64)
    R, w = _float_gaussian(sigma)
    err = np.abs(g[:R + 1] / 256.0 - w)
    e1 = err[0] + 2.0 * err[1:].sum()
    S = g[0] + 2 * g[1:].sum()
    bound = 2.0 * e1 + S / 65536.0
    i = np.arange(28)
    dist = np.abs(i[:, None] - i[None, :])
    G64 = np.where(dist <= R, w[np.minimum(dist, R)], 0.0)
    N = elastic_noise(elastic_key(SEED, step, [j]))[0]
    F, _ = elastic_field(g, N)
    worst = np.abs(F / 32768.0 - G64 @ (N / 128.0) @ G64.T).max()
    print(f"sigma {sigma} step {step} j {j}: {worst:.3e} bound {bound:.3e}")
    assert worst <= bound


@pytest.mark.parametrize("sigma", [1.0, 4.0, 16.0])
def test_range_on_the_extreme_fields_and_identity_at_zero_alpha(sigma):
    g = elastic_taps(sigma)
    for v in (-128, 127):
        F, T8 = elastic_field(g, np.full((2, 28, 28), v))
        assert -128 <= T8.min() and T8.max() <= 127
        assert np.abs(F).max() <= 32768
    rng = np.random.RandomState(3)
    rows = torch.from_numpy(rng.randint(0, 256, (5, 784), dtype=np.uint8))
    ent = torch.from_numpy(augment_table(5, SEED, 4, 20, 0.3))
    assert torch.equal(
        elastic_warp_u8(rows, ent, elastic_displacement(g, 0, SEED, 3, 5)),
        affine_warp_u8(rows, ent))
    dS = elastic_displacement(g, 16384, SEED, 3, 5)
    assert dS.any() and np.abs(dS).max() <= 1 << 23


def test_field_is_a_pure_function_of_seed_step_and_position():
    g = elastic_taps(4.0)
    a = elastic_displacement(g, 8704, SEED, 5, 4)
    assert np.array_equal(a, elastic_displacement(g, 8704, SEED, 5, 4))
    assert len({x.tobytes() for x in a}) == 4               # j matters
    assert not np.array_equal(a, elastic_displacement(g, 8704, SEED, 6, 4))
    assert not np.array_equal(
        a, elastic_displacement(g, 8704, SEED, 5 + (1 << 32), 4))
    rng = np.random.RandomState(1)
    img = rng.randint(0, 256, (40, 784), dtype=np.uint8)
    lab = rng.randint(0, 10, 40, dtype=np.uint8)
    ds = DeviceDataSet(img, lab, seed=SEED, augment_elastic=34)
    assert ds.aug_table.shape == (1, 6) and ds.elastic[1] == 8704
    x, y = ds.batch_at(9, 8)
    rx, ry = ds.batch_at(9, 8, augment=False)
    assert torch.equal(y, ry) and not torch.equal(x, rx)
    rows = ((rx.reshape(8, 784) * 255 + 127.5).round()).to(torch.uint8)
    want = elastic_warp_u8(rows, ds.aug_table.expand(8, 6),
                           elastic_displacement(g, 8704, SEED, 9, 8))
    assert torch.equal(x.reshape(8, 784), ds._lut[want.long()])


def test_argument_errors(tmp_path):
    from distributedmnist_amd.engine.train import make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    for bad in (0.5, 16.5, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            elastic_taps(bad)
    for bad in (np.full(32, 8), np.r_[128, np.zeros(31, int)],
                np.r_[-1, np.zeros(31, int)], np.zeros(31, int)):
        with pytest.raises(ValueError):
            cpu_ref.check_elastic_taps(bad)
    img = np.zeros((4, 784), dtype=np.uint8)
    lab = np.zeros(4, dtype=np.uint8)
    for kw in ({"augment_elastic": -1.0}, {"augment_elastic": 65.0},
               {"augment_elastic": float("nan")},
               {"augment_elastic": 8.0, "augment_elastic_sigma": 0.5},
               {"augment_elastic": 8.0, "augment_elastic_sigma": float("nan")}):
        with pytest.raises(ValueError):
            DeviceDataSet(img, lab, **kw)
    write_random_idx(str(tmp_path / "data"), 64, 8, seed=1)
    base = ["--data_dir", str(tmp_path / "data"), "--train_dir",
            str(tmp_path / "td"), "--device", "cpu"]
    parse = build_train_parser().parse_args
    for bad in (["--augment_elastic", "-1"], ["--augment_elastic", "nan"],
                ["--augment_elastic", "65"],
                ["--augment_elastic_sigma", "0.5"]):
        with pytest.raises(SystemExit):
            parse(base + bad)
    for extra in ([], ["--synthetic_data"], ["--device_data", "--fake_data"]):
        with pytest.raises(ValueError, match="--augment_elastic"):
            make_dataset(parse(base + extra + ["--augment_elastic", "34"]),
                         0, 1, torch.device("cpu"), torch.float32)
    ds = make_dataset(parse(base + ["--device_data", "--augment_elastic",
                                    "34", "--augment_shift", "2"]),
                      0, 1, torch.device("cpu"), torch.float32)
    assert ds.elastic[1] == 8704 and ds.aug_table.shape == (4096, 6)
