"""Top-k sparsification on the GPU (--grad_topk): the kernels of
csrc/topk.hip against the exact CPU reference, bit for bit, and deterministic
trainer runs, graphed and eager."""

import pytest
import torch
from test_clip_gpu import LENET_NUMELS, bits

from distributedmnist_amd.ops import cpu_ref
from distributedmnist_amd.ops import functional as Fx

pytestmark = pytest.mark.gpu

# contiguous and adversarial: segments that straddle the 4096-element chunks,
# several segments in one chunk, lengths that are no multiple of 4
TABLES = {"lenet": LENET_NUMELS, "odd": [1, 3, 4097, 63, 8197, 10]}
PAD = 8


def family(name, n, numels, gen):
    if name == "normal":
        return torch.randn(n, generator=gen)
    if name == "ties":  # massive ties across blocks: tie-by-index, need_eq
        return torch.tensor([0, .5, -.5, 1, -1, 2, -2])[
            torch.randint(0, 7, (n,), generator=gen)]
    if name == "zeros":
        return torch.zeros(n)
    if name == "last_digit":  # keys that differ in the low radix digits only
        return (1 + torch.randperm(n, generator=gen).double() * 2.0 ** -23
                ).float()
    g = torch.zeros(n)  # "spike": one huge element among zeros
    big = max(range(len(numels)), key=lambda t: numels[t])
    g[sum(numels[:big]) + numels[big] // 2] = -3e30
    return g


@pytest.mark.parametrize("fam", ["normal", "ties", "zeros", "last_digit",
                                 "spike"])
@pytest.mark.parametrize("ratio", [1e-9, 0.01, 0.5, 1.0])
@pytest.mark.parametrize("table", list(TABLES))
def test_compress_matches_cpu_reference(table, ratio, fam):
    numels = TABLES[table]
    offs = [sum(numels[:i]) for i in range(len(numels))]
    n = sum(numels)
    ks = cpu_ref.topk_ks(numels, ratio)
    assert ratio > 1e-9 or ks == [1] * len(numels)
    gen = torch.Generator().manual_seed(11)
    r_ref = torch.zeros(n)
    bufs = [torch.full((n + PAD,), 7.5, device="cuda") for _ in range(2)]
    g_dev, r_dev = bufs[0][:n], bufs[1][:n]  # canaries behind both
    r_dev.zero_()
    for step in range(3):  # fresh gradients, the residual carries
        g = family(fam, n, numels, gen)
        pay_ref, dense_ref = cpu_ref.topk_compress(g, r_ref, offs, numels, ks)
        g_dev.copy_(g)
        pay, out = Fx.topk_compress(g_dev, r_dev, offs, numels, ks)
        assert out.data_ptr() == g_dev.data_ptr()
        assert torch.equal(pay.cpu(), pay_ref), (step, "payload")
        assert torch.equal(bits(r_dev), bits(r_ref)), (step, "residual")
        assert torch.equal(bits(g_dev), bits(dense_ref)), (step, "bucket")
    assert all(bool((b[n:] == 7.5).all()) for b in bufs)
    # the multi-rank form: same pairs and residual, a zeroed bucket
    g_dev.copy_(g)
    r_dev.copy_(r_ref)
    r2 = r_ref.clone()
    pay_ref, _ = cpu_ref.topk_compress(g, r2, offs, numels, ks)
    pay, _ = Fx.topk_compress(g_dev, r_dev, offs, numels, ks, dense=False)
    assert torch.equal(pay.cpu(), pay_ref) and not bool(g_dev.any())
    assert torch.equal(bits(r_dev), bits(r2))


def test_scatter_adds_in_rank_order():
    numels = TABLES["odd"]
    offs = [sum(numels[:i]) for i in range(len(numels))]
    n = sum(numels)
    ks = cpu_ref.topk_ks(numels, 0.5)  # half of everything: ranks overlap
    gen = torch.Generator().manual_seed(3)
    pays = torch.stack([
        cpu_ref.topk_compress(torch.randn(n, generator=gen) * 10.0 ** w,
                              torch.zeros(n), offs, numels, ks)[0]
        for w in range(3)])
    want = cpu_ref.topk_scatter(pays, n)
    assert torch.equal(bits(Fx.topk_scatter(pays.cuda(), n)), bits(want))
    other = cpu_ref.topk_scatter(pays.flip(0), n)
    assert not torch.equal(bits(other), bits(want))  # the order matters


B, STEPS = 64, 4


def trainer_run(tmp_path, graph, monkeypatch):
    from distributedmnist_amd import _C
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    argv = ["--synthetic_data", "--model", "lenet", "--deterministic",
            "--batch_size", str(B), "--max_steps", str(STEPS),
            "--grad_topk", "0.01", "--momentum", "0.9",
            "--save_interval_secs", "100000", "--train_dir",
            str(tmp_path / ("graph" if graph else "eager"))]
    argv += [] if graph else ["--hip_graph", "off"]
    flags = build_train_parser().parse_args(argv)
    real = Fx.topk_compress

    def checked(g, r, *args, **kw):
        """bucket-before-update + residual = old residual + local gradient"""
        want = r + g
        out = real(g, r, *args, **kw)
        assert torch.equal(g + r, want) and not bool(((g != 0) & (r != 0)).any())
        return out
    if not graph:
        monkeypatch.setattr(Fx, "topk_compress", checked)
    try:
        t = Trainer(flags, device=torch.device("cuda:0"))
        ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
        for _ in range(STEPS):
            x, y = ds.next_batch(B)
            _, loss, _, _ = t.graph_or_eager_step(x, y)
            assert float(loss) == float(loss)
        torch.cuda.synchronize()
        assert (t._graph is not None) == graph, "capture must engage"
        stats = t.topk_stats()
        assert [v[0] for v in stats.values()] == t.topk_ks
        assert all(v[1] > 0 and 0 < v[2] < 1 for v in stats.values())
        return t.fp.flat_master.cpu(), t.flat_topk_residual.cpu()
    finally:
        _C.ext().set_deterministic(False)


def test_graphed_and_eager_trainers_agree_bitwise(tmp_path, monkeypatch):
    graphed = trainer_run(tmp_path, True, monkeypatch)
    eager = trainer_run(tmp_path, False, monkeypatch)
    for a, b in zip(graphed, eager):
        assert torch.equal(bits(a), bits(b)) and bool(a.any())
