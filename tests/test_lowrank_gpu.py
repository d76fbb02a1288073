"""PowerSGD compression on the GPU (--grad_lowrank): the kernels of
csrc/lowrank.hip against float64 replays of the same fp32 inputs, the
bucket layout, and deterministic trainer runs, graphed and eager."""

import math

import pytest
import torch
from test_clip_gpu import bits

from distributedmnist_amd.ops import cpu_ref
from distributedmnist_amd.ops import functional as Fx

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PAD = 8
# the tile minimum, one and many row slices of the Q kernel, one and eight
# column groups, rows that are no multiple of the 128-row slice, the maximum
SHAPES = [(64, 64), (800, 64), (784, 512), (3136, 512), (4096, 64)]
LENET = [(5, 5, 1, 32), (32,), (5, 5, 32, 64), (64,), (3136, 512), (512,),
         (512, 10), (10,)]


def make_state(shapes, R, pack=False):
    """a LowrankState whose buffers have canaries behind them"""
    offs = [sum(math.prod(s) for s in shapes[:i]) for i in range(len(shapes))]
    n = sum(math.prod(s) for s in shapes)
    st = Fx.LowrankState(shapes, offs, n, R, 5, "cuda", pack)
    bufs = [torch.full((n + PAD,), 7.5, device="cuda")]
    for name in ("resid", "q", "qr", "wire"):
        src = getattr(st, name)
        bufs.append(torch.full((src.numel() + PAD,), 7.5, device="cuda"))
        bufs[-1][:src.numel()] = src
        setattr(st, name, bufs[-1][:src.numel()])
    if not pack:
        st.qr = st.q
    return st, bufs[0][:n], bufs


def gradient(fam, rows, cols, gen):
    if fam == "normal":
        return torch.randn(rows, cols, generator=gen)
    # exactly rank 2 in fp32: small-integer factors
    return (torch.randint(-4, 5, (rows, 2), generator=gen).float()
            @ torch.randint(-4, 5, (2, cols), generator=gen).float())


def fro(a, b):
    return float(torch.linalg.matrix_norm(a.double().cpu() - b.double().cpu()))


@pytest.mark.parametrize("fam", ["normal", "rank2"])
@pytest.mark.parametrize("R", [1, 4, 16])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_kernels_against_float64(rows, cols, R, fam):
    """P and Q_r: elementwise (K + 4) * 2^-24 * |A| |B| against the float64
    product of the same fp32 operands.  P^ and the bucket: Frobenius error
    against the float64 replay at most 3x that of the fp32 torch reference,
    for P^ plus 4 * 2^-24 * |P^| (docs/KERNELS.md "Low-rank compression"
    records the measured ratios).
    World 1: bucket + E = M within 2 * 2^-24 * (|M| + |bucket|), which needs
    the product to be formed once."""
    st, g, bufs = make_state([(rows, cols)], R)
    gen = torch.Generator().manual_seed(rows + cols + R)
    for step in range(3):  # the residual and the warm-started Q carry
        G = gradient(fam, rows, cols, gen)
        E0, Q0 = st.resid.view(rows, cols).clone(), st.q.view(cols, R).clone()
        g.copy_(G.reshape(-1))
        Fx.lowrank_p(g, st)
        M = st.resid.view(rows, cols).clone()
        assert torch.equal(bits(M), bits(G.cuda() + E0)), step
        P = st.wire.view(rows, R).clone()
        err = (P.double() - M.double() @ Q0.double()).abs()
        assert bool((err <= (cols + 4) * U * (M.abs().double()
                                              @ Q0.abs().double())).all()), step
        Fx.lowrank_q(st)
        Ph, Qr = st.wire.view(rows, R).clone(), st.q.view(cols, R).clone()
        want = cpu_ref.lowrank_orth(P.double().cpu())
        e_ref = fro(cpu_ref.lowrank_orth(P.cpu()), want)
        e_gpu = fro(Ph, want)
        print(f"orth {rows}x{cols} R={R} {fam} step {step}: gpu {e_gpu:.3e} "
              f"ref {e_ref:.3e}")
        # + 4 roundings of the column's one scale (last add of the norm,
        # sqrt, + 1e-8, divide): a matter of luck in any fp32 result, so not
        # proportional to the reference's error
        assert e_gpu <= 3 * e_ref + 4 * U * float(
            torch.linalg.matrix_norm(want)), (step, "orth", e_gpu, e_ref)
        err = (Qr.double() - M.double().t() @ Ph.double()).abs()
        assert bool((err <= (rows + 4) * U * (M.abs().double().t()
                                              @ Ph.abs().double())).all()), step
        Fx.lowrank_expand(g, st)
        bucket, E = g.view(rows, cols), st.resid.view(rows, cols)
        b64 = cpu_ref.lowrank_step(G.double(), E0.double().cpu(),
                                   Q0.double().cpu())[0]
        e_ref = fro(cpu_ref.lowrank_step(G, E0.cpu(), Q0.cpu())[0], b64)
        e_gpu = fro(bucket, b64)
        print(f"bucket {rows}x{cols} R={R} {fam} step {step}: gpu "
              f"{e_gpu:.3e} ref {e_ref:.3e}")
        assert e_gpu <= 3 * e_ref, (step, "bucket", e_gpu, e_ref)
        assert bool(((bucket + E - M).abs()
                     <= 2 * U * (M.abs() + bucket.abs())).all()), step
    assert all(bool((b[-PAD:] == 7.5).all()) for b in bufs)


@pytest.mark.parametrize("pack", [False, True])
def test_lenet_layout_passes_dense_tensors_through(pack):
    """dense tensors before, between and after the two compressed ones keep
    their bits and a zero residual; packing them behind P and unpacking them
    (the multi-rank route, here without a second rank) changes nothing"""
    st, g, bufs = make_state(LENET, 4, pack)
    assert [(p[0], p[2], p[3]) for p in st.plan] == [(2, 800, 64),
                                                     (4, 3136, 512)]
    G = torch.randn(st.n, generator=torch.Generator().manual_seed(2)).cuda()
    dense = torch.ones(st.n, dtype=torch.bool, device="cuda")
    for t in range(2):
        st.views(dense, t).fill_(False)
    assert int(dense.sum()) == st.dense_floats == 6538
    g.copy_(G)
    Fx.lowrank_p(g, st)
    Fx.lowrank_q(st)
    if pack:
        st.q.copy_(st.qr)
        g[dense] = -1.0  # the unpacking has to restore them
    Fx.lowrank_expand(g, st)
    assert torch.equal(bits(g[dense]), bits(G[dense]))
    assert not bool(st.resid[dense].any()) and bool(st.resid[~dense].any())
    assert all(bool((b[-PAD:] == 7.5).all()) for b in bufs)
    # both routes: the same bits as the CPU form's structure, M conserved
    assert bool(((g + st.resid - G).abs()[~dense]
                 <= 2 * U * (G.abs() + g.abs())[~dense]).all())


B, STEPS = 64, 8


def trainer_run(tmp_path, tag, graph):
    from distributedmnist_amd import _C
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    argv = ["--synthetic_data", "--model", "lenet", "--deterministic",
            "--batch_size", str(B), "--max_steps", str(STEPS),
            "--grad_lowrank", "4", "--momentum", "0.9",
            "--save_interval_secs", "100000", "--train_dir",
            str(tmp_path / tag)]
    argv += [] if graph else ["--hip_graph", "off"]
    flags = build_train_parser().parse_args(argv)
    try:
        t = Trainer(flags, device=torch.device("cuda:0"))
        ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
        for _ in range(STEPS):
            x, y = ds.next_batch(B)
            _, loss, _, _ = t.graph_or_eager_step(x, y)
            assert float(loss) == float(loss)
        torch.cuda.synchronize()
        assert (t._graph is not None) == graph, "capture must engage"
        stats = t.lowrank_stats()
        assert sorted(stats) == ["conv2_w", "fc1_w"]
        assert all(r == 4 and 0 < share < 1 for r, share in stats.values())
        return (t.fp.flat_master.cpu(), t.flat_lowrank_residual.cpu(),
                t.flat_lowrank_q.cpu())
    finally:
        _C.ext().set_deterministic(False)


def test_graphed_and_eager_trainers_agree_bitwise(tmp_path):
    """under --deterministic, where the gradients themselves repeat"""
    runs = [trainer_run(tmp_path, tag, graph) for tag, graph in
            (("graph", True), ("again", True), ("eager", False))]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(bits(a), bits(b)) and bool(a.any())
