"""Top-k sparsification with error feedback (--grad_topk), CPU side: the
invariants of the exact reference, the refused flag combinations, and trainer
runs at world 1 and on two gloo ranks."""

import pytest
import torch
from mp_utils import init_pg, spawn_collect

from distributedmnist_amd.ops import cpu_ref
from distributedmnist_amd.utils.flags import build_train_parser

NUMELS = [1, 3, 4097, 63, 8197, 10]
OFFSETS = [sum(NUMELS[:i]) for i in range(len(NUMELS))]
# min(n, max(1, ceil(ratio * n)))
KS = {1e-6: [1] * 6, 0.01: [1, 1, 41, 1, 82, 1],
      0.5: [1, 2, 2049, 32, 4099, 5], 1.0: NUMELS}


@pytest.mark.parametrize("ratio", [1e-6, 0.01, 0.5, 1.0])
@pytest.mark.parametrize("family", ["normal", "ties"])
def test_reference_invariants(ratio, family):
    n = sum(NUMELS)
    gen = torch.Generator().manual_seed(5)
    ks = cpu_ref.topk_ks(NUMELS, ratio)
    assert ks == KS[ratio] and cpu_ref.topk_ks([0], ratio) == [0]
    r = torch.zeros(n)
    for _ in range(3):  # the residual carries
        if family == "normal":
            g = torch.randn(n, generator=gen)
        else:
            g = torch.tensor([0, .5, -.5, 1, -1, 2, -2])[
                torch.randint(0, 7, (n,), generator=gen)]
        a = r + g
        payload, dense = cpu_ref.topk_compress(g, r, OFFSETS, NUMELS, ks)
        assert torch.equal(dense + r, a)
        assert not bool(((dense != 0) & (r != 0)).any())
        base = 0
        for o, m, k in zip(OFFSETS, NUMELS, ks):
            idx = payload[0, base:base + k].long()
            assert bool((idx[1:] > idx[:-1]).all())  # ascending, so unique
            assert o <= int(idx[0]) and int(idx[-1]) < o + m
            assert torch.equal(payload[1, base:base + k],
                               a.view(torch.int32)[idx])
            # nothing left behind beats anything sent
            left = a[o:o + m].abs().clone()
            left[idx - o] = -1.0
            assert float(left.max()) <= float(a[idx].abs().min())
            base += k
        assert base == payload.shape[1]
        assert torch.equal(cpu_ref.topk_scatter(payload[None], n), dense)


@pytest.mark.parametrize("argv", [
    ["--grad_topk", "-0.1"], ["--grad_topk", "1.5"], ["--grad_topk", "nan"],
    ["--grad_topk", "0.1", "--interval_method"],
    ["--grad_topk", "0.1", "--straggler_timeout_ms", "5"],
    ["--grad_topk", "0.1", "--grad_dtype", "bf16"]])
def test_refused_flags_are_argument_errors(argv, capsys):
    with pytest.raises(SystemExit) as ei:
        build_train_parser().parse_args(argv)
    assert ei.value.code == 2
    assert "--grad_topk" in capsys.readouterr().err


@pytest.mark.parametrize("extra,world", [
    (["--num_replicas_to_aggregate", "1"], 2), (["--hip_graph", "full"], 2)])
def test_refused_at_start_up(tmp_path, extra, world):
    from distributedmnist_amd.engine.train import Trainer
    flags = build_train_parser().parse_args(
        ["--synthetic_data", "--train_dir", str(tmp_path), "--device", "cpu",
         "--model", "mlp", "--grad_topk", "0.1"] + extra)
    with pytest.raises(ValueError, match="--grad_topk cannot be combined"):
        Trainer(flags, rank=0, world=world)


def run_trainer(train_dir, rank=0, world=1, extra=()):
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    flags = build_train_parser().parse_args(
        ["--synthetic_data", "--train_dir", train_dir, "--device", "cpu",
         "--model", "mlp", "--batch_size", "16", "--momentum", "0.9",
         "--save_interval_secs", "100000", *extra])
    t = Trainer(flags, rank=rank, world=world, local_rank=rank)
    ds = make_dataset(flags, rank, world, t.device, t.compute_dtype)
    for _ in range(3):
        assert t.train_step(*t.to_device(*ds.next_batch(16)))[0]
    return t


def test_world1_full_ratio_is_the_dense_run(tmp_path):
    off = run_trainer(str(tmp_path / "off"))
    full = run_trainer(str(tmp_path / "full"), extra=("--grad_topk", "1.0"))
    part = run_trainer(str(tmp_path / "part"), extra=("--grad_topk", "0.05"))
    assert torch.equal(full.fp.flat_master, off.fp.flat_master)
    assert not bool(full.flat_topk_residual.any())
    assert not torch.equal(part.fp.flat_master, off.fp.flat_master)
    assert bool(part.flat_topk_residual.any())
    assert "flat_topk_residual" in part.checkpoint_payload()
    stats = part.topk_stats()
    for name, k in zip(part.fp.names, part.topk_ks):
        assert stats[name][0] == k and stats[name][1] >= 0
        assert 0 < stats[name][2] <= 1
    with pytest.raises(RuntimeError, match="grad_topk"):
        off.topk_stats()


def _rank_train(rank, world, port, train_dir, extra, q):
    import torch.distributed as dist
    init_pg(rank, world, port)
    t = run_trainer(train_dir, rank, world, extra)
    q.put((rank, t.fp.flat_master.numpy().tobytes()))
    dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_world2_ranks_agree_and_full_ratio_is_dense(tmp_path):
    out = {tag: spawn_collect(_rank_train, 2,
                              args=(str(tmp_path / tag), extra))
           for tag, extra in (("part", ("--grad_topk", "0.05")),
                              ("full", ("--grad_topk", "1.0")),
                              ("dense", ()))}
    for res in out.values():
        assert res[0] == res[1]  # both ranks hold the same bits
    # every element sent, and a two-term sum commutes
    assert out["full"][0] == out["dense"][0]
    assert out["part"][0] != out["dense"][0]
