"""MXFP8 gradient wire on the GPU (--grad_dtype mxfp8): the kernels of
csrc/mxwire.hip against the exact CPU reference, bit for bit, and trainer
runs, graphed and eager."""

import numpy as np
import pytest
import torch
from test_clip_gpu import bits

from distributedmnist_amd.ops import cpu_ref
from distributedmnist_amd.ops import functional as Fx

pytestmark = pytest.mark.gpu

PAD = 64


def crafted(n):
    """Every branch of the scale byte and of the rounding, cut to n."""
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(max(n, 16384) + 5, generator=gen) * 0.01
    blk = x[:32 * 12].view(12, 32)
    blk[1] = 0.0                                     # all-zero block
    blk[2, 3] = 448 * 2.0 ** -9                      # amax = 448 * 2^k
    blk[3, 5] = float(np.nextafter(np.float32(448 * 2.0 ** -9), np.float32(1)))
    blk[4] = torch.arange(1, 33).float() * 1e-42     # fp32 subnormals only
    blk[5, 0], blk[5, 1] = 1e-39, -3e-45             # subnormals below an amax
    blk[6, 7] = 430.0 * 2.0 ** -5                    # (416, 448] * 2^e
    blk[7, 31] = 3e38
    blk[8, 0], blk[8, 9] = float("nan"), float("inf")
    blk[9, 2], blk[9, 3] = 2.0 ** -100, -2.0 ** -120  # y underflows the grid
    blk[10, 1] = -3.4e38                             # may round to -inf
    return x[:n].contiguous()


@pytest.fixture(scope="module")
def reference():
    """(n, W) -> (x, wire) of the crafted vector, computed once."""
    out = {}
    for n in (1, 33, 16389):
        x = crafted(n)
        enc = cpu_ref.mx_encode(x, 66478, (1 << 33) + 5, 0, 2)
        for W in (1, 3):
            out[n, W] = (x, cpu_ref.mx_to_wire(*enc, W))
    return out


@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("n", [1, 33, 16389])
def test_encode_matches_cpu_reference(reference, n, W):
    x, want = reference[n, W]
    buf = torch.full((want.numel() + PAD,), 0xA5, dtype=torch.uint8,
                     device="cuda")  # canary behind the wire
    keep = torch.full((n + PAD,), 7.5, device="cuda")
    step_dev = torch.tensor([(1 << 33) + 5], device="cuda")
    wire = Fx.mx_encode(x.cuda(), 66478, 0, 0, 2, world=W,
                        out=buf[:want.numel()].view(W, -1), keep=keep[:n],
                        step_dev=step_dev)
    assert torch.equal(wire.cpu(), want)
    assert bool((buf[want.numel():] == 0xA5).all())
    assert torch.equal(bits(keep[:n]), bits(x)) and bool((keep[n:] == 7.5).all())


@pytest.mark.parametrize("W", [2, 3, 8])
def test_reduce_matches_cpu_reference(W):
    n = 16389 // 3  # one shard: 171 blocks, padded to 176
    gen = torch.Generator().manual_seed(W)
    rows = torch.stack([
        cpu_ref.mx_to_wire(*cpu_ref.mx_encode(
            torch.randn(n, generator=gen) * 10.0 ** (r - 2), 1, 9, 0, r), 1)[0]
        for r in range(W)])
    rows[W - 1, 32 * 176 + 5] = 0xFF  # one NaN block from the last rank
    want = cpu_ref.mx_reduce(rows, 1, 9, W - 1)
    got = Fx.mx_reduce(rows.cuda(), 1, 9, W - 1)
    assert torch.equal(got.cpu(), want) and int(want[32 * 176 + 5]) == 0xFF


@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("n", [1, 33, 16389])
def test_decode_is_exact_and_stays_inside(reference, n, W):
    wire = reference[n, W][1]
    codes, scales = (t.numpy().astype(np.int64)
                     for t in cpu_ref.mx_from_wire(wire))
    mant, ex = codes & 7, (codes >> 3) & 15
    with np.errstate(over="ignore"):
        want = np.where(ex == 0, mant * 2.0 ** -9,
                        (8 + mant) * 2.0 ** (ex - 10.0))
        want = (np.where(codes & 0x80, -want, want)
                * 2.0 ** (np.repeat(scales, 32) - 127.0))
        want = np.where(np.repeat(scales, 32) == 0xFF, np.nan, want)
        want = torch.from_numpy(want.astype(np.float32)[:n])
    out = torch.full((n + PAD,), 7.5, device="cuda")
    Fx.mx_decode(wire.cuda(), n, out=out[:n])
    got = out[:n].cpu()
    assert torch.equal(got.isnan(), want.isnan())
    assert torch.equal(bits(got.nan_to_num(0.0)), bits(want.nan_to_num(0.0)))
    assert bool((out[n:] == 7.5).all())


B, STEPS = 64, 3


def trainer_run(tmp_path, graph):
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    argv = ["--synthetic_data", "--model", "lenet", "--batch_size", str(B),
            "--max_steps", str(STEPS), "--grad_dtype", "mxfp8",
            "--deterministic", "--momentum", "0.9",
            "--save_interval_secs", "100000", "--train_dir",
            str(tmp_path / ("graph" if graph else "eager"))]
    argv += [] if graph else ["--hip_graph", "off"]
    flags = build_train_parser().parse_args(argv)
    from distributedmnist_amd import _C
    try:
        t = Trainer(flags, device=torch.device("cuda:0"))
        ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
        for _ in range(STEPS):
            _, loss, _, _ = t.graph_or_eager_step(*ds.next_batch(B))
            assert float(loss) == float(loss)
        torch.cuda.synchronize()
        assert (t._graph is not None) == graph, "capture must engage"
        stats = t.mx_stats()
        assert list(stats) == t.fp.names
        assert all(0 < v < 2.0 ** -3 for v in stats.values()), stats
        return t.fp.flat_master.cpu()
    finally:
        _C.ext().set_deterministic(False)


def test_graphed_and_eager_trainers_agree_bitwise(tmp_path):
    graphed, eager = trainer_run(tmp_path, True), trainer_run(tmp_path, False)
    assert torch.equal(bits(graphed), bits(eager)) and bool(graphed.any())
