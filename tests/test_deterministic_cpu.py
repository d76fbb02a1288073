"""--deterministic on the CPU: the reference form of the ordered plane
reduction, the flag, the three timing-mode conflicts, and the flag being a
no-op for CPU training (which is bitwise deterministic as it is)."""

import numpy as np
import pytest
import torch

from distributedmnist_amd.ops import cpu_ref
from distributedmnist_amd.utils.flags import build_train_parser


def mixed(shape, seed):
    """normal x 10^U(-3, 3): magnitudes mixed enough that order changes bits."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) *
            10.0 ** (6.0 * torch.rand(shape, generator=g) - 3.0))


@pytest.mark.parametrize("P", [1, 2, 7])
@pytest.mark.parametrize("n", [1, 10, 133])
def test_plane_reduce_is_the_sequential_fp32_loop(P, n):
    planes = mixed((P, n), 100 * P + n)
    out0 = mixed((n,), 7 * P + n)
    pn, on = planes.numpy(), out0.numpy()
    want = np.empty(n, dtype=np.float32)
    for i in range(n):
        s = np.float32(pn[0, i])
        for p in range(1, P):
            s = np.float32(s + np.float32(pn[p, i]))
        want[i] = np.float32(np.float32(on[i]) + s)
    out = out0.clone()
    ret = cpu_ref.plane_reduce(planes, out)
    assert ret is out
    assert np.array_equal(out.numpy().view(np.int32), want.view(np.int32))


def test_plane_reduce_order_matters_on_this_data():
    planes = mixed((7, 4096), 3)
    a = cpu_ref.plane_reduce(planes, torch.zeros(4096))
    b = cpu_ref.plane_reduce(planes.flip(0), torch.zeros(4096))
    assert not torch.equal(a, b)


def test_plane_reduce_writes_through_a_view():
    planes = mixed((3, 5), 11)
    big = torch.zeros(8)
    cpu_ref.plane_reduce(planes, big[1:6])
    assert torch.equal(big[1:6], (planes[0] + planes[1]) + planes[2])
    assert float(big[0]) == 0.0 and bool((big[6:] == 0).all())


def test_flag_parsing():
    p = build_train_parser()
    assert p.parse_args([]).deterministic is False
    assert p.parse_args(["--deterministic"]).deterministic is True


def _flags(tmp_path, *extra):
    return build_train_parser().parse_args(
        ["--synthetic_data", "--train_dir", str(tmp_path), "--batch_size",
         "16", "--max_steps", "3", "--save_interval_secs", "100000",
         "--device", "cpu", *extra])


@pytest.mark.parametrize("extra,world,needle", [
    (["--interval_method"], 1, "--interval_method"),
    (["--num_replicas_to_aggregate", "1"], 2, "--num_replicas_to_aggregate"),
    (["--straggler_timeout_ms", "5"], 1, "--straggler_timeout_ms"),
])
def test_timing_modes_conflict(tmp_path, extra, world, needle):
    from distributedmnist_amd.engine.train import Trainer, check_deterministic
    flags = _flags(tmp_path, "--deterministic", *extra)
    with pytest.raises(ValueError, match="--deterministic") as ei:
        check_deterministic(flags, torch.device("cpu"), torch.float32, world)
    assert needle in str(ei.value)
    if world == 1:
        with pytest.raises(ValueError, match="--deterministic"):
            Trainer(flags, device=torch.device("cpu"))
    # without the flag the same settings are accepted
    flags_off = _flags(tmp_path, *extra)
    assert flags_off.deterministic is False


def test_full_aggregation_is_not_a_conflict(tmp_path):
    from distributedmnist_amd.engine.train import check_deterministic
    for k in ("-1", "2", "3"):
        flags = _flags(tmp_path, "--deterministic",
                       "--num_replicas_to_aggregate", k)
        check_deterministic(flags, torch.device("cpu"), torch.float32, 2)


def _train_cpu(tmp_path, tag, *extra):
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    flags = _flags(tmp_path / tag, *extra)
    t = Trainer(flags, device=torch.device("cpu"))
    ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
    losses = []
    for _ in range(3):
        x, y = ds.next_batch(16)
        _, loss, _, _ = t.train_step(x, y)
        losses.append(float(loss))
    return t.fp.flat_master.clone(), losses


def test_cpu_training_is_unchanged_by_the_flag(tmp_path):
    w0, l0 = _train_cpu(tmp_path, "off")
    w1, l1 = _train_cpu(tmp_path, "on", "--deterministic")
    assert l0 == l1
    assert torch.equal(w0.view(torch.int32), w1.view(torch.int32))
