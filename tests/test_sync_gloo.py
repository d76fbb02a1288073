"""Multi-process (gloo, world_size=2) tests of the sync engine — the
distributed path is made correct-by-construction here on CPU; the same code
runs over RCCL on the 8-GPU node (SURVEY.md section 4 item c)."""

import os  # noqa: F401  (children use env)

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp  # noqa: F401

from distributedmnist_amd.parallel.sync import SyncEngine

from mp_utils import free_port, init_pg, spawn_collect  # noqa: F401


def _init(rank, world, port):
    init_pg(rank, world, port)


def _run_full_sync(rank, world, port, q):
    _init(rank, world, port)
    g = torch.full((10,), float(rank + 1))
    eng = SyncEngine(g, mode="full_sync", rank=rank, world_size=world)
    eng.step_begin(0)
    applied, grad, contributors = eng.reduce(0, 0.01)
    q.put((rank, applied, grad[0].item(), contributors))
    dist.destroy_process_group()


def _run_k_of_n(rank, world, port, q):
    _init(rank, world, port)
    g = torch.full((10,), float(rank + 1))
    eng = SyncEngine(g, mode="k_of_n", replicas_to_aggregate=1,
                     rank=rank, world_size=world)
    eng.step_begin(0)
    # rank 1 is the slow one -> excluded with K=1
    applied, grad, contributors = eng.reduce(0, compute_time_s=0.01 + rank)
    q.put((rank, applied, grad[0].item(), contributors))
    dist.destroy_process_group()


def _run_interval(rank, world, port, q):
    _init(rank, world, port)
    g = torch.full((4,), 1.0)
    eng = SyncEngine(g, mode="interval", interval_ms=0.0,
                     rank=rank, world_size=world)
    # interval_ms=0 -> fires on every step; 2 ranks x grad=1 accumulated once
    eng.step_begin(0)
    applied, grad, contributors = eng.reduce(0, 0.01)
    q.put((rank, applied, None if grad is None else grad[0].item(), contributors))
    dist.destroy_process_group()


def _run_timeout(rank, world, port, q):
    _init(rank, world, port)
    g = torch.full((4,), float(rank + 1))
    eng = SyncEngine(g, mode="full_sync", straggler_timeout_ms=100.0,
                     rank=rank, world_size=world)
    eng.step_begin(0)
    # rank 1 exceeds the 100ms deadline -> drops its own contribution
    ct = 0.01 if rank == 0 else 0.5
    applied, grad, contributors = eng.reduce(0, compute_time_s=ct)
    q.put((rank, applied, grad[0].item(), contributors))
    dist.destroy_process_group()


def _spawn(fn, world=2, args=()):
    return spawn_collect(fn, world, args=args)


@pytest.mark.timeout(120)
def test_full_sync_sums_and_counts():
    res = _spawn(_run_full_sync)
    for r in (0, 1):
        applied, gval, contributors = res[r]
        assert applied and contributors == 2
        assert gval == 3.0  # 1 + 2 summed; engine returns SUM


@pytest.mark.timeout(120)
def test_k_of_n_drops_slowest():
    res = _spawn(_run_k_of_n)
    for r in (0, 1):
        applied, gval, contributors = res[r]
        assert applied and contributors == 1
        assert gval == 1.0  # only rank 0 (fast) contributed


@pytest.mark.timeout(120)
def test_interval_fires_and_averages():
    res = _spawn(_run_interval)
    for r in (0, 1):
        applied, gval, contributors = res[r]
        assert applied and contributors == 2
        assert gval == 2.0  # both accumulators (1 step each) summed


@pytest.mark.timeout(120)
def test_straggler_timeout_drops_self():
    res = _spawn(_run_timeout)
    for r in (0, 1):
        applied, gval, contributors = res[r]
        assert applied and contributors == 1
        assert gval == 1.0  # rank 1's grad zeroed


def _run_interval_freerun(rank, world, port, q):
    import time
    _init(rank, world, port)
    g = torch.ones(1000)
    eng = SyncEngine(g, mode="interval", interval_ms=50.0,
                     rank=rank, world_size=world)
    steps = 30
    t0 = time.time()
    for s in range(steps):
        eng.step_begin(s)
        if rank == 1:
            time.sleep(0.05)  # 10x+ slower rank
        eng.reduce(s, 0.01)
    loop_time = time.time() - t0
    for _grad, _c in eng.finalize_interval():
        pass
    q.put((rank, loop_time, eng.generation, eng._gen_posted,
           float(eng.flat_grad.sum())))
    dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_interval_slow_rank_does_not_stall_fast_rank():
    """VERDICT round-1 task 3 'done' criterion: with free-running interval
    aggregation a 10x-slower rank must NOT stall the fast rank between
    firings (the reference's workers never block between interval updates,
    distributed_train.py:271-288)."""
    res = _spawn(_run_interval_freerun)
    fast_loop, slow_loop = res[0][0], res[1][0]
    assert slow_loop >= 1.2          # 30 x 50ms injected sleep
    # fast rank's stepping loop is decoupled: it must finish far before the
    # slow rank (the round-1 per-step broadcast made these equal)
    assert fast_loop < 0.5 * slow_loop, (fast_loop, slow_loop)
    # after the drain both ranks posted and applied identical generations
    assert res[0][1] == res[1][1] > 0    # generation (applied)
    assert res[0][2] == res[1][2]        # gen_posted
    assert res[0][3] == res[1][3]        # same final aggregated grad


def _run_interval_3rank(rank, world, port, q):
    """3 ranks with DIFFERENT speeds + jitter: the generation agreement and
    ring backpressure must hold for any relative timing."""
    import random
    import time
    _init(rank, world, port)
    rng = random.Random(1000 + rank)
    g = torch.ones(512)
    eng = SyncEngine(g, mode="interval", interval_ms=25.0,
                     rank=rank, world_size=world)
    for s in range(24):
        eng.step_begin(s)
        time.sleep(rng.uniform(0, 0.012) * (rank + 1))
        eng.reduce(s, 0.001)
    for _grad, _c in eng.finalize_interval():
        pass
    q.put((rank, eng.generation, eng._gen_posted,
           float(eng.flat_grad.sum())))
    dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_interval_3rank_jittered_agreement():
    res = _spawn(_run_interval_3rank, world=3)
    gens = {res[r][0] for r in range(3)}
    posted = {res[r][1] for r in range(3)}
    finals = {res[r][2] for r in range(3)}
    assert len(gens) == 1 and len(posted) == 1, (gens, posted)
    assert res[0][0] > 0, "no aggregation ever fired"
    assert len(finals) == 1, finals  # same aggregated grad everywhere


def _run_trainer_interval_e2e(rank, world, port, train_dir, q):
    _init(rank, world, port)
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    flags = build_train_parser().parse_args(
        ["--synthetic_data", "--train_dir", train_dir,
         "--batch_size", "16", "--max_steps", "25", "--model", "mlp",
         "--device", "cpu", "--interval_method", "--interval_ms", "40",
         "--inject_slow_rank", "1", "--inject_slow_ms", "25"])
    t = Trainer(flags, rank=rank, world=world, local_rank=rank)
    ds = make_dataset(flags, rank, world, t.device, t.compute_dtype)
    t.train(ds)
    q.put((rank, t.engine.generation, t.fp.flat_master.sum().item(),
           t.fp.flat_master[:5].tolist()))
    dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_trainer_interval_e2e_params_identical_after_drain(tmp_path):
    res = _spawn(_run_trainer_interval_e2e, args=(str(tmp_path / "td"),))
    assert res[0] == res[1], "ranks diverged in interval mode"
    assert res[0][0] > 0, "no interval aggregation ever fired"


def _run_bf16_wire(rank, world, port, q):
    _init(rank, world, port)
    torch.manual_seed(100 + rank)
    g32 = torch.randn(4096)
    g16 = g32.clone()
    e32 = SyncEngine(g32, mode="full_sync", rank=rank, world_size=world)
    e16 = SyncEngine(g16, mode="full_sync", rank=rank, world_size=world,
                     wire_dtype=torch.bfloat16)
    assert e16._buf.dtype == torch.bfloat16  # wire payload IS bf16 (half size)
    e32.step_begin(0)
    _, r32, c32 = e32.reduce(0, 0.01)
    e16.step_begin(0)
    _, r16, c16 = e16.reduce(0, 0.01)
    err = float((r32 - r16).abs().max())
    scale = float(r32.abs().max())
    q.put((rank, err, scale, c32, c16))
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_bf16_wire_allreduce_parity():
    """--grad_dtype bf16: half wire payload, result within bf16 rounding of
    the fp32 reduce (fp32 master update unchanged)."""
    res = _spawn(_run_bf16_wire)
    for r in (0, 1):
        err, scale, c32, c16 = res[r]
        assert c32 == c16 == 2
        assert err <= 0.02 * scale, (err, scale)


def _run_dc_pre(rank, world, port, q):
    _init(rank, world, port)
    from distributedmnist_amd.ops import functional as Fx
    g = torch.ones(4096)
    Fx.grad_mask(g, 0.9, seed=66478, step=3, rank=rank)
    my_kept = float((g != 0).float().mean())
    eng = SyncEngine(g, mode="full_sync", rank=rank, world_size=world)
    eng.step_begin(0)
    _, agg, _ = eng.reduce(0, 0.01)
    hist = [float((agg == v).float().mean()) for v in (0.0, 1.0, 2.0)]
    q.put((rank, my_kept, hist))
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_drop_connect_pre_aggregation_masks_are_rank_distinct():
    """VERDICT round-1 task 4: each rank masks its OWN gradient before the
    all-reduce (reference distributed_train.py:194-203).  With keep=0.9 and
    grad=1 everywhere, the aggregated values are 0/1/2 with ~1% zeros, ~18%
    ones, ~81% twos — the 'ones' bucket only exists if the masks differ."""
    res = _spawn(_run_dc_pre)
    for r in (0, 1):
        kept, hist = res[r]
        assert 0.86 < kept < 0.94
        p0, p1, p2 = hist
        assert p1 > 0.10, f"masks identical across ranks? ones={p1}"
        assert abs(p0 - 0.01) < 0.02 and abs(p2 - 0.81) < 0.05
        assert abs(p0 + p1 + p2 - 1.0) < 1e-6


def _run_trainer_e2e(rank, world, port, train_dir, q):
    _init(rank, world, port)
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    flags = build_train_parser().parse_args(
        ["--synthetic_data", "--train_dir", train_dir,
         "--batch_size", "16", "--max_steps", "5", "--model", "mlp",
         "--device", "cpu"])
    t = Trainer(flags, rank=rank, world=world, local_rank=rank)
    ds = make_dataset(flags, rank, world, t.device, t.compute_dtype)
    t.train(ds)
    q.put((rank, t.fp.flat_master.sum().item(),
           t.fp.flat_master[:5].tolist()))
    dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_trainer_e2e_params_identical_across_ranks(tmp_path):
    res = _spawn(_run_trainer_e2e, args=(str(tmp_path / "td"),))
    assert res[0] == res[1], "ranks diverged after 5 sync steps"


def _run_k_of_n_tie(rank, world, port, q):
    _init(rank, world, port)
    g = torch.full((10,), float(rank + 1))
    eng = SyncEngine(g, mode="k_of_n", replicas_to_aggregate=1,
                     rank=rank, world_size=world)
    eng.step_begin(0)
    # EQUAL compute times: the (time, rank) sort key must break the tie
    # identically on every rank (rank 0 wins) or the contribute decisions
    # diverge and the renormalization count is wrong
    applied, grad, contributors = eng.reduce(0, compute_time_s=0.5)
    q.put((rank, applied, grad[0].item(), contributors))
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_k_of_n_tie_break_deterministic():
    res = _spawn(_run_k_of_n_tie)
    for r in (0, 1):
        applied, gval, contributors = res[r]
        assert applied and contributors == 1
        assert gval == 1.0  # rank 0 wins the tie on both ranks
