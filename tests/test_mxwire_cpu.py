"""MXFP8 gradient wire (--grad_dtype mxfp8), CPU side: the flag and its
refusals, the properties of the exact reference, and two gloo ranks against a
single-process replay through the reference."""

import numpy as np
import pytest
import torch
from mp_utils import init_pg, spawn_collect

from distributedmnist_amd.ops import cpu_ref
from distributedmnist_amd.utils.flags import build_train_parser

BASE = ["--synthetic_data", "--device", "cpu", "--model", "mlp",
        "--batch_size", "16", "--save_interval_secs", "100000",
        "--grad_dtype", "mxfp8"]


def test_parser_accepts_mxfp8():
    assert build_train_parser().parse_args(BASE).grad_dtype == "mxfp8"


@pytest.mark.parametrize("argv", [
    ["--interval_method"], ["--straggler_timeout_ms", "5"],
    ["--grad_topk", "0.1"], ["--grad_lowrank", "2"]])
def test_refused_flags_are_argument_errors(argv, capsys):
    with pytest.raises(SystemExit) as ei:
        build_train_parser().parse_args(BASE + argv)
    assert ei.value.code == 2
    assert "mxfp8" in capsys.readouterr().err


@pytest.mark.parametrize("extra", [
    ["--num_replicas_to_aggregate", "1"], ["--hip_graph", "full"]])
def test_refused_at_start_up(tmp_path, extra):
    from distributedmnist_amd.engine.train import Trainer
    flags = build_train_parser().parse_args(
        BASE + ["--train_dir", str(tmp_path)] + extra)
    with pytest.raises(ValueError, match="mxfp8 cannot be combined"):
        Trainer(flags, rank=0, world=2)


def grid_step(dec, scales):
    """One e4m3 grid step at |y|, times 2^e, per element: 2^(k - 3) for |y|
    in [2^k, 2^(k + 1)), k >= -6, and 2^-9 below."""
    e = np.repeat(scales.numpy().astype(np.int64) - 127, 32)
    y = np.abs(np.ldexp(dec.double().numpy(), -e))
    k = np.maximum(np.frexp(np.maximum(y, 2.0 ** -6))[1] - 1, -6)
    return np.ldexp(1.0, k - 3 + e)


def test_reference_error_bound_and_idempotence():
    gen = torch.Generator().manual_seed(11)
    # magnitudes across the normal, e4m3-subnormal and vanishing ranges
    x = torch.randn(4099, generator=gen) * torch.exp2(
        torch.randint(-20, 4, (4099,), generator=gen).float())
    codes, scales = cpu_ref.mx_encode(x, 3, 5, 0, 1)
    dec = cpu_ref.mx_decode(codes, scales)
    xp = torch.zeros_like(dec)
    xp[:4099] = x
    # |y| lies between two neighbouring grid points of its own binade (the
    # binade bounds are grid points), one grid step apart, and the decoded
    # value is one of the two
    err = (dec.double() - xp.double()).abs().numpy()
    assert bool((err < grid_step(xp, scales)).all())
    # already on the grid: nothing left to round, whatever the key (a block
    # whose amax was rounded down to 224 * 2^e takes the next smaller scale
    # and a finer grid, so the values are compared, not the bytes)
    again = cpu_ref.mx_decode(*cpu_ref.mx_encode(dec, 99, 7, 1, 0))
    assert torch.equal(again, dec)
    wire = cpu_ref.mx_to_wire(codes, scales, 1)
    one = cpu_ref.mx_reduce(wire, 4, 4, 0)
    one = cpu_ref.mx_decode(*cpu_ref.mx_from_wire(one))  # with padding blocks
    assert torch.equal(one[:dec.numel()], dec) and not one[dec.numel():].any()


def test_reference_is_unbiased():
    x = torch.randn(64, generator=torch.Generator().manual_seed(2))
    d = torch.stack([cpu_ref.mx_decode(*cpu_ref.mx_encode(x, 17, s, 0, 0))
                     for s in range(4096)]).double()
    se = d.std(dim=0) / 4096 ** 0.5
    off = (d.mean(dim=0) - x.double()).abs()
    assert bool((off <= 5 * se).all()), (off / se.clamp_min(1e-30)).max()


def make_trainer(train_dir, rank, world):
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    flags = build_train_parser().parse_args(
        BASE + ["--train_dir", train_dir, "--momentum", "0.9"])
    t = Trainer(flags, rank=rank, world=world, local_rank=rank)
    return t, make_dataset(flags, rank, world, t.device, t.compute_dtype)


def _rank_train(rank, world, port, train_dir, q):
    import torch.distributed as dist
    init_pg(rank, world, port)
    t, ds = make_trainer(train_dir, rank, world)
    for _ in range(6):
        assert t.train_step(*t.to_device(*ds.next_batch(16)))[0]
    assert all(0 <= v < 2.0 ** -3 for v in t.mx_stats().values())
    q.put((rank, t.fp.flat_master.numpy().tobytes()))
    dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_world2_ranks_agree_with_the_reference_replay(tmp_path):
    res = spawn_collect(_rank_train, 2, args=(str(tmp_path / "dist"),))
    assert res[0] == res[1]  # both ranks hold the same bits
    # the same run in one process: local gradients as train_step computes
    # them, the exchange through cpu_ref alone
    ranks = [make_trainer(str(tmp_path / f"replay{r}"), r, 2)
             for r in range(2)]
    seed = ranks[0][0].flags.seed
    n = ranks[0][0].fp.flat_grad.numel()
    for step in range(6):
        wires = []
        for r, (t, ds) in enumerate(ranks):
            x, y = t.to_device(*ds.next_batch(16))
            t.model.set_step(step)
            t.fp.zero_grad()
            loss, _ = t.model.loss_and_accuracy(t.model(x, train=True), y)
            loss.backward()
            t.fp.fix_grad_views()
            wires.append(cpu_ref.mx_to_wire(
                *cpu_ref.mx_encode(t.fp.flat_grad, seed, step, 0, r), 2))
        shards = torch.stack([
            cpu_ref.mx_reduce(torch.stack([w[o] for w in wires]), seed, step,
                              o) for o in range(2)])
        total = cpu_ref.mx_decode(*cpu_ref.mx_from_wire(shards))[:n]
        for t, _ in ranks:
            t.fp.flat_grad.copy_(total)
            t._apply_update(t.fp.flat_grad, 2)
            t.step += 1
    assert ranks[0][0].fp.flat_master.numpy().tobytes() == res[0][0]
