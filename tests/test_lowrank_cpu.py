"""PowerSGD compression with error feedback (--grad_lowrank), CPU side: the
plan, the algebra of the reference in float64, two gloo ranks, the refused
flag combinations and the checkpoint keys."""

import math

import pytest
import torch
from mp_utils import init_pg, spawn_collect

from distributedmnist_amd.ops import cpu_ref
from distributedmnist_amd.utils.flags import build_train_parser

LENET = [(5, 5, 1, 32), (32,), (5, 5, 32, 64), (64,), (3136, 512), (512,),
         (512, 10), (10,)]
MLP = [(784, 512), (512,), (512, 10), (10,)]


def offsets(shapes):
    return [sum(math.prod(s) for s in shapes[:i]) for i in range(len(shapes))]


@pytest.mark.parametrize("shapes,want", [
    (LENET, [(2, 832, 800, 64), (4, 52096, 3136, 512)]),
    (MLP, [(0, 0, 784, 512)]),
    # an odd-length vector in front: the matrix's offset is no multiple of 4
    ([(3,), (64, 64)], []),
    ([(4,), (64, 64), (48, 64), (64, 72), (4112, 64), (64, 528)],
     [(1, 4, 64, 64)])])
def test_plan(shapes, want):
    assert cpu_ref.lowrank_plan(shapes, offsets(shapes), 4) == want


def test_plan_refuses_a_fifth_tensor_and_bad_ranks():
    with pytest.raises(ValueError, match="at most 4"):
        cpu_ref.lowrank_plan([(64, 64)] * 5, offsets([(64, 64)] * 5), 4)
    for R in (0, 17):
        with pytest.raises(ValueError, match="1..16"):
            cpu_ref.lowrank_plan(MLP, offsets(MLP), R)


@pytest.mark.parametrize("rank2", [False, True])
def test_reference_algebra_in_float64(rank2):
    """Against a replay written out here.  Full rank: P^ is orthonormal up
    to the 1e-8 in its norms and bucket + E = M.  Exact rank 2 under R = 4:
    bucket = M and E = 0, because a dependent column is left as float64
    rounding noise, which the 1e-8 in its norm keeps small."""
    gen = torch.Generator().manual_seed(3)
    rows, cols, R = 96, 80, 4
    if rank2:
        M = (torch.randn(rows, 2, generator=gen, dtype=torch.float64)
             @ torch.randn(2, cols, generator=gen, dtype=torch.float64))
    else:
        M = torch.randn(rows, cols, generator=gen, dtype=torch.float64)
    E = 0.25 * M
    G = M - E
    Q = torch.randn(cols, R, generator=gen, dtype=torch.float64)
    bucket, E1, Q1, Ph = cpu_ref.lowrank_step(G, E, Q)
    P = (G + E) @ Q
    for i in range(R):  # the replay: classic column-by-column form
        P[:, i] /= P[:, i].norm() + 1e-8
        for j in range(i + 1, R):
            P[:, j] -= (P[:, i] @ P[:, j]) / (P[:, i] @ P[:, i]) * P[:, i]
    Qr = (G + E).t() @ P
    scale = float(M.norm())
    assert torch.allclose(bucket + E1, M, rtol=0, atol=1e-12)
    if rank2:
        # noise of 1e-16 |P| over 1e-8 leaves a column of at most 1e-6
        assert float((bucket - M).norm()) <= 1e-6 * scale
        assert float(E1.norm()) <= 1e-6 * scale
        return
    assert torch.allclose(Ph, P, rtol=0, atol=1e-12)
    assert torch.allclose(Q1, Qr, rtol=0, atol=1e-10)
    assert torch.allclose(bucket, P @ Qr.t(), rtol=0, atol=1e-10)
    # columns of norm >= 1: 1e-8 moves each Gram entry by a few 1e-8
    assert torch.allclose(Ph.t() @ Ph, torch.eye(R, dtype=torch.float64),
                          rtol=0, atol=1e-6)


@pytest.mark.parametrize("argv", [
    ["--grad_lowrank", "-1"], ["--grad_lowrank", "17"],
    ["--grad_lowrank", "2.5"],
    ["--grad_lowrank", "2", "--grad_topk", "0.1"],
    ["--grad_lowrank", "2", "--interval_method"],
    ["--grad_lowrank", "2", "--straggler_timeout_ms", "5"],
    ["--grad_lowrank", "2", "--grad_dtype", "bf16"]])
def test_refused_flags_are_argument_errors(argv, capsys):
    with pytest.raises(SystemExit) as ei:
        build_train_parser().parse_args(argv)
    assert ei.value.code == 2
    assert "--grad_lowrank" in capsys.readouterr().err


@pytest.mark.parametrize("extra,world", [
    (["--num_replicas_to_aggregate", "1"], 2), (["--hip_graph", "full"], 2)])
def test_refused_at_start_up(tmp_path, extra, world):
    from distributedmnist_amd.engine.train import Trainer
    flags = build_train_parser().parse_args(
        ["--synthetic_data", "--train_dir", str(tmp_path), "--device", "cpu",
         "--model", "mlp", "--grad_lowrank", "2"] + extra)
    with pytest.raises(ValueError, match="--grad_lowrank cannot be combined"):
        Trainer(flags, rank=0, world=world)


def run_trainer(train_dir, rank=0, world=1, extra=(), steps=6):
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    flags = build_train_parser().parse_args(
        ["--synthetic_data", "--train_dir", train_dir, "--device", "cpu",
         "--model", "mlp", "--batch_size", "16", "--momentum", "0.9",
         "--save_interval_secs", "100000", *extra])
    t = Trainer(flags, rank=rank, world=world, local_rank=rank)
    ds = make_dataset(flags, rank, world, t.device, t.compute_dtype)
    for _ in range(steps):
        assert t.train_step(*t.to_device(*ds.next_batch(16)))[0]
    return t


def test_checkpoint_keys_and_stats(tmp_path):
    on = run_trainer(str(tmp_path / "on"), extra=("--grad_lowrank", "2"),
                     steps=2)
    off = run_trainer(str(tmp_path / "off"), steps=1)
    p = on.checkpoint_payload()
    assert p["flat_lowrank_residual"].shape == on.fp.flat_grad.shape
    assert p["flat_lowrank_q"].shape == (2 * 512,)
    assert bool(p["flat_lowrank_residual"][:784 * 512].any())
    assert not bool(p["flat_lowrank_residual"][784 * 512:].any())
    q = off.checkpoint_payload()
    assert q["flat_lowrank_residual"] is None and q["flat_lowrank_q"] is None
    (name, (rank, share)), = on.lowrank_stats().items()
    assert name == "fc1_w" and rank == 2 and 0 < share < 1
    with pytest.raises(RuntimeError, match="grad_lowrank"):
        off.lowrank_stats()


def _rank_train(rank, world, port, train_dir, q):
    import torch.distributed as dist
    from distributedmnist_amd.ops import functional as Fx
    init_pg(rank, world, port)
    t = run_trainer(train_dir, rank, world, ("--grad_lowrank", "2"))
    master = t.fp.flat_master.numpy().tobytes()
    # one more exchange by hand, from a zero residual, on a known gradient
    g = torch.randn(t.fp.flat_grad.numel(),
                    generator=torch.Generator().manual_seed(rank))
    t.lowrank.resid.zero_()
    q0 = t.lowrank.q.clone()
    t.fp.flat_grad.copy_(g)
    Fx.lowrank_p(t.fp.flat_grad, t.lowrank)
    t.engine.lowrank_exchange()
    # bytes: a tensor in the queue would need this process to stay alive
    q.put((rank, master) + tuple(x.numpy().tobytes()
                                 for x in (g, q0, t.fp.flat_grad)))
    dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_world2_ranks_agree_and_sum_is_projected(tmp_path):
    out = spawn_collect(_rank_train, 2, args=(str(tmp_path),))
    assert out[0][0] == out[1][0]  # both ranks hold the same parameters
    assert out[0][2] == out[1][2]  # and the same warm-started Q
    out = {r: [torch.frombuffer(bytearray(b), dtype=torch.float32)
               for b in v] for r, v in out.items()}
    # from zero residuals the bucket is the single-process step on the summed
    # gradient; the dense tensors are summed exactly
    n = 784 * 512
    total = out[0][1] + out[1][1]
    want = cpu_ref.lowrank_step(total[:n].view(784, 512),
                                torch.zeros(784, 512),
                                out[0][2].view(512, 2))[0]
    for r in range(2):
        got = out[r][3]
        assert torch.equal(got[n:], total[n:])
        # fp32 sums in another order: 784 + 2 terms of 2^-24 each
        assert torch.allclose(got[:n].view(784, 512), want, rtol=0,
                              atol=786 * 2.0 ** -24 * float(want.abs().max()))
