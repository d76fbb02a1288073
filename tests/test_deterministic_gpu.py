"""Deterministic mode on the GPU (ext.set_deterministic / --deterministic):
the seven gradient flush sites of the fused LeNet step store per-block planes
and plane_reduce adds them in index order.

"Repeatable" = ten calls from identical inputs into fresh zeroed destinations,
every odd call issued while a 2048^2 torch.mm runs on a second stream (to
perturb block scheduling), all ten results torch.equal.

Inputs, references and tolerances of the value checks are the ones of the
tests that cover the default route: test_pool2_bwd_fused_gpu.py (conv2 dW),
test_conv1_mfma_gpu.py (conv1 dW+db, softmax), test_fc1_epilogues_gpu.py
(fc dW bound, bias-grad bound)."""

import pytest
import torch

import test_conv1_mfma_gpu as c1
import test_pool2_bwd_fused_gpu as p2
from distributedmnist_amd.ops import cpu_ref

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
SWITCHES = ("DMNIST_DW2_SLAB", "DMNIST_DW2_G", "DMNIST_DW2_KHB",
            "DMNIST_DW2_NBUF", "DMNIST_DW_G", "DMNIST_DW_SPREAD",
            "DMNIST_DW1_G", "DMNIST_DW1_SLAB", "DMNIST_DW_PLAN",
            "DMNIST_DW_TR", "DMNIST_CONV1_VALU", "DMNIST_UNPOOL_TILE",
            "DMNIST_UNPOOL_LINES", "DMNIST_POOL2_FUSED", "DMNIST_OVERLAP",
            "DMNIST_TWO_STREAM", "DMNIST_SINGLE_STREAM",
            "DMNIST_EAGER_FUSED")


@pytest.fixture(scope="module")
def ext():
    from distributedmnist_amd import _C
    m = _C.ext()
    assert m is not None, "HIP extension must be present on GPU boxes"
    return m


@pytest.fixture(autouse=True)
def det(ext, monkeypatch):
    """Default dispatch, switch on for the test, off again on exit."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    ext.set_deterministic(True)
    yield
    ext.set_deterministic(False)


_MM = {}


def repeatable(fn, n=10):
    """fn() -> tuple of tensors; returns the first result."""
    if "a" not in _MM:
        _MM["a"] = torch.randn(2048, 2048, device="cuda")
        _MM["s"] = torch.cuda.Stream()
    a, side = _MM["a"], _MM["s"]
    outs = []
    for i in range(n):
        if i % 2:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                torch.mm(a, a)
                torch.mm(a, a)
        outs.append(tuple(t.clone() for t in fn()))
    torch.cuda.synchronize()
    for i, o in enumerate(outs[1:], 1):
        for j, (x, y) in enumerate(zip(outs[0], o)):
            assert torch.equal(x, y), f"call {i} output {j} differs"
    return outs[0]


def mixed(shape, seed):
    """normal x 10^U(-3, 3), CPU fp32."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) *
            10.0 ** (6.0 * torch.rand(shape, generator=g) - 3.0))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def view_of(n, aligned):
    """A zeroed fp32 [n] destination: a fresh tensor, or a view that starts at
    element 1 of a larger one (not 16 B aligned)."""
    if aligned:
        return torch.zeros(n, device="cuda")
    v = torch.zeros(n + 5, device="cuda")[1:1 + n]
    assert v.data_ptr() % 16 != 0
    return v


# ---------------------------------------------------------------------------
# 1. plane_reduce is the formula
# ---------------------------------------------------------------------------
_PLANES = {}


def planes_case(P, n):
    if (P, n) not in _PLANES:
        pl = mixed((P, n), 1000 * P + n)
        c = mixed((n,), 77 * P + n)
        want = cpu_ref.plane_reduce(pl, c.clone())
        _PLANES[(P, n)] = (pl, c, want)
    return _PLANES[(P, n)]


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("n", [1, 10, 832, 51200, 51203])
@pytest.mark.parametrize("P", [1, 2, 5, 86, 257])
def test_plane_reduce_is_the_formula(ext, P, n, aligned):
    pl, c, want = planes_case(P, n)
    out = view_of(n, aligned)
    out.copy_(c)
    ext.plane_reduce(pl.cuda(), out)
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(want))


def test_plane_data_is_order_sensitive():
    pl, _, _ = planes_case(86, 51200)
    a = cpu_ref.plane_reduce(pl, torch.zeros(51200))
    b = cpu_ref.plane_reduce(pl.flip(0), torch.zeros(51200))
    assert not torch.equal(a, b)


def test_plane_reduce_rejects_bad_arguments(ext):
    with pytest.raises(RuntimeError):
        ext.plane_reduce(torch.zeros(2, 8, device="cuda"),
                         torch.zeros(9, device="cuda"))
    with pytest.raises(RuntimeError):
        ext.plane_reduce(torch.zeros(2, 8, device="cuda", dtype=bf16),
                         torch.zeros(8, device="cuda"))


# ---------------------------------------------------------------------------
# the seven sites: one runner each, (inputs) -> callable(dest...) -> outputs
# ---------------------------------------------------------------------------
def conv2_run(ext, nb):
    x, gp, am, _, _ = p2.case(nb)

    def run(dw):
        ext.conv_dw_pooled_into(x, gp, am, dw)
        return (dw,)
    return run, (p2.NOUT,)


_C1 = {}


def conv1_case(nb):
    if nb not in _C1:
        x, dyp, am = c1.dw_inputs(nb, "random", 7 * nb + 1)
        _C1[nb] = (x, dyp, am) + tuple(c1.dw_ref_fp64(x, dyp, am))
    return _C1[nb]


def conv1_run(ext, nb):
    x, dyp, am, _, _ = conv1_case(nb)

    def run(dw, db):
        ext.conv1_dw_pooled(x, dyp, am, dw, db)
        return dw, db
    return run, (800, 32)


_FC = {}


def fc_case(K, N, B):
    if (K, N, B) not in _FC:
        g = torch.Generator().manual_seed(K * 7 + N * 3 + B)
        x = torch.randn(B, K, generator=g).to(bf16).cuda()
        dy = (torch.randn(B, N, generator=g) * 0.1).to(bf16).cuda()
        ref = x.double().t() @ dy.double()
        mag = x.float().abs().t() @ dy.float().abs()
        _FC[(K, N, B)] = (x, dy, ref, mag)
    return _FC[(K, N, B)]


def fc_run(ext, K, N, B):
    x, dy, _, _ = fc_case(K, N, B)

    def run(dw):
        ext.linear_dw_into(x, dy, dw)
        return (dw,)
    return run, (K * N,)


def softmax_run(ext, B):
    logits, labels = c1.softmax_case(B)
    lg, lb = logits.cuda(), labels.cuda()

    def run(db):
        loss, acc, dl = ext.softmax_xent_fwd(lg, lb, db_out=db, inv_n=1.0 / B)
        return db, loss, acc, dl
    return run, (10,)


_MASK = {}


def mask_case(B):
    if B not in _MASK:
        g = torch.Generator(device="cuda").manual_seed(300 + B)
        dyeff = (torch.randn((B, 10), device="cuda", generator=g)
                 * 0.1).to(bf16)
        w = (torch.randn((512, 10), device="cuda", generator=g)
             * 0.05).to(bf16)
        actm = torch.randn((B, 512), device="cuda", generator=g).to(bf16)
        _MASK[B] = (dyeff, w, actm)
    return _MASK[B]


def mask_run(ext, B):
    dyeff, w, actm = mask_case(B)

    def run(db):
        dx = ext.linear_dx_mask(dyeff, w, actm, db, 0.5)
        return db, dx
    return run, (512,)


_POOLED = {}
KP = p2.HO * p2.WO * p2.COUT


def pooled_case(B):
    if B not in _POOLED:
        g = torch.Generator(device="cuda").manual_seed(B * 1000 + 64)
        dyeff = (torch.randn((B, 64), device="cuda", generator=g)
                 * 0.1).to(bf16)
        w = (torch.randn((KP, 64), device="cuda", generator=g)
             * 0.05).to(bf16)
        am = p2.draw_am((B, p2.HO, p2.WO, p2.COUT), g)
        _POOLED[B] = (dyeff, w, am)
    return _POOLED[B]


def pooled_run(ext, B, tile=0):
    dyeff, w, am = pooled_case(B)

    def run(db):
        gp = ext.linear_dx_pooled(dyeff, w, am, db, p2.HO, p2.WO, p2.COUT,
                                  tile=tile)
        return db, gp
    return run, (p2.COUT,)


def fresh(sizes, aligned=True):
    return [view_of(n, aligned) for n in sizes]


# ---------------------------------------------------------------------------
# 2. conv2 dW pooled
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nb,g", [(1, None), (5, None), (130, None),
                                  (515, None), (64, "1")])
def test_conv2_dw(ext, monkeypatch, nb, g):
    if g is not None:
        monkeypatch.setenv("DMNIST_DW2_G", g)
    if nb == 515:
        assert int(ext.conv2_dw_group(nb)) == 12     # 43 groups, 5 padded
    run, sizes = conv2_run(ext, nb)
    (dw,) = repeatable(lambda: run(*fresh(sizes)))
    p2.check(f"det NB={nb}", dw, p2.case(nb)[4])


@pytest.mark.parametrize("nb", [5, 130])
def test_conv2_dw_dense_slab_route_is_covered(ext, nb):
    """conv_dw_into on the conv2 slab route shares the pooled kernel's flush
    and is covered, not refused."""
    x, _, _, dact, ref = p2.case(nb)

    def run():
        dw = torch.zeros(p2.NOUT, device="cuda")
        ext.conv_dw_into(x, dact, dw)
        return (dw,)
    (dw,) = repeatable(run)
    p2.check(f"det dense NB={nb}", dw, ref)


def test_conv_dw_into_off_the_slab_route_raises(ext, monkeypatch):
    x, _, _, dact, _ = p2.case(5)
    monkeypatch.setenv("DMNIST_DW2_SLAB", "0")
    with pytest.raises(RuntimeError, match="conv_dw_into"):
        ext.conv_dw_into(x, dact, torch.zeros(p2.NOUT, device="cuda"))


# ---------------------------------------------------------------------------
# 3. conv1 dW + db
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nb,g", [(1, None), (3, None), (515, None),
                                  (40, "16")])
def test_conv1_dw_db(ext, monkeypatch, nb, g):
    if g is not None:
        monkeypatch.setenv("DMNIST_DW1_G", g)
    run, sizes = conv1_run(ext, nb)
    dw, db = repeatable(lambda: run(*fresh(sizes)))
    _, _, _, dw64, db64 = conv1_case(nb)
    c1.check_dw(f"det NB={nb}", dw, db, dw64, db64)


# ---------------------------------------------------------------------------
# 4. fc dW
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("K,N,B,plan,want_split", [
    (3136, 512, 64, None, 1), (3136, 512, 1600, None, 2),
    (3136, 512, 320, "128,128,5", 5), (512, 10, 1, None, None),
    (512, 10, 257, None, None), (200, 72, 300, None, None)])
def test_fc_dw(ext, monkeypatch, K, N, B, plan, want_split, aligned):
    if plan is not None:
        monkeypatch.setenv("DMNIST_DW_PLAN", plan)
    tbm, bn, sk = ext.linear_dw_plan(K, N, B)
    if want_split is not None:
        assert sk == want_split, (tbm, bn, sk)
    run, sizes = fc_run(ext, K, N, B)
    (dw,) = repeatable(lambda: run(*fresh(sizes, aligned)))
    _, _, ref, mag = fc_case(K, N, B)
    bound = 8.0 * (B + 8) * 2.0 ** -24 * mag.double()
    err = (dw.view(K, N).double() - ref).abs()
    print("plan", (tbm, bn, sk), "max err/bound",
          float((err / bound.clamp(min=1e-30)).max()))
    assert bool((err <= bound).all())


# ---------------------------------------------------------------------------
# 5. the three bias gradients
# ---------------------------------------------------------------------------
def off_mode(ext, run, sizes):
    ext.set_deterministic(False)
    try:
        out = tuple(t.clone() for t in run(*fresh(sizes)))
    finally:
        ext.set_deterministic(True)
    return out


def check_db(db, db_off, terms, sum_abs, exact):
    # the bias-grad bound of test_fc1_epilogues_gpu.py / test_pool2_bwd_fused:
    # two kernels summing the same fp32 terms in another order
    bound = 2.0 * terms * 2.0 ** -24 * sum_abs
    diff = (db - db_off).abs()
    print("db det-vs-default max diff", float(diff.max()), "bound min",
          float(bound.min()))
    assert bool((diff <= bound).all())
    scale = float(exact.abs().max().clamp(min=1e-3))
    torch.testing.assert_close(db, exact.float(), rtol=2e-2,
                               atol=0.02 * scale)


@pytest.mark.parametrize("B", [1, 257, 1000])
def test_softmax_db(ext, B):
    run, sizes = softmax_run(ext, B)
    db, loss, acc, dl = repeatable(lambda: run(*fresh(sizes)))
    db0, loss0, acc0, dl0 = off_mode(ext, run, sizes)
    assert torch.equal(loss, loss0) and torch.equal(acc, acc0)
    assert torch.equal(dl.view(torch.int16), dl0.view(torch.int16))
    exact = dl.double().sum(dim=0)
    # d values are rounded to bf16 in dl: allow that on top of the order
    sum_abs = dl.float().abs().sum(dim=0) * (1 + 2.0 ** -7)
    check_db(db, db0, B, sum_abs, exact)


@pytest.mark.parametrize("B", [1, 65, 129])
def test_linear_dx_mask_db(ext, B):
    run, sizes = mask_run(ext, B)
    db, dx = repeatable(lambda: run(*fresh(sizes)))
    db0, dx0 = off_mode(ext, run, sizes)
    assert torch.equal(dx.view(torch.int16), dx0.view(torch.int16))
    dyeff, w, actm = mask_case(B)
    g = (dyeff.float() @ w.float().t()) * (actm.float() > 0) * 2.0
    check_db(db, db0, B, g.abs().sum(dim=0), g.double().sum(dim=0))


@pytest.mark.parametrize("tile", [0, 64, 128])
@pytest.mark.parametrize("B", [1, 65, 129, 700])
def test_linear_dx_pooled_db(ext, B, tile):
    if B == 700:
        assert int(ext.linear_dx_pooled_tile(B, KP)) == 128
    run, sizes = pooled_run(ext, B, tile)
    db, gp = repeatable(lambda: run(*fresh(sizes)))
    db0, gp0 = off_mode(ext, run, sizes)
    assert torch.equal(gp.view(torch.int16), gp0.view(torch.int16))
    dyeff, w, am = pooled_case(B)
    g = ((dyeff.float() @ w.float().t()).view(B, p2.HO, p2.WO, p2.COUT)
         * (am < 4))
    check_db(db, db0, B * p2.HO * p2.WO, g.abs().sum(dim=(0, 1, 2)),
             g.double().sum(dim=(0, 1, 2)))


# ---------------------------------------------------------------------------
# 6. accumulate contract: out = fl(c + g), one fp32 add
# ---------------------------------------------------------------------------
SITES = {
    "softmax_db": lambda e: softmax_run(e, 257),
    "fc1_b": lambda e: mask_run(e, 129),
    "conv2_b_64": lambda e: pooled_run(e, 129, 64),
    "conv2_b_128": lambda e: pooled_run(e, 129, 128),
    "fc1_dw_split": lambda e: fc_run(e, 3136, 512, 1600),
    "fc2_dw": lambda e: fc_run(e, 512, 10, 257),
    "conv2_dw": lambda e: conv2_run(e, 130),
    "conv1_dw_db": lambda e: conv1_run(e, 515),
}


@pytest.mark.parametrize("site", sorted(SITES))
def test_accumulates_with_one_add(ext, site):
    run, sizes = SITES[site](ext)
    g = [t.clone() for t in run(*fresh(sizes))[:len(sizes)]]
    gen = torch.Generator(device="cuda").manual_seed(len(site))
    c = [torch.randn(n, device="cuda", generator=gen) for n in sizes]
    dest = [t.clone() for t in c]
    got = run(*dest)[:len(sizes)]
    torch.cuda.synchronize()
    for gi, ci, oi in zip(g, c, got):
        assert bool((gi != 0).any())
        assert torch.equal(bits(oi), bits(ci + gi))


# ---------------------------------------------------------------------------
# 7. nothing stale is read
# ---------------------------------------------------------------------------
STALE = {
    "conv2_dw_nb1": lambda e: conv2_run(e, 1),       # 1 real + 7 padded groups
    "conv2_dw_nb515": lambda e: conv2_run(e, 515),   # 43 real + 5 padded
    "conv1_dw_db": lambda e: conv1_run(e, 515),
    "fc1_dw_split": lambda e: fc_run(e, 3136, 512, 1600),
    "fc2_dw": lambda e: fc_run(e, 512, 10, 257),
    "fc_ragged": lambda e: fc_run(e, 200, 72, 300),
    "softmax_db": lambda e: softmax_run(e, 1000),
    "fc1_b": lambda e: mask_run(e, 65),
    "conv2_b": lambda e: pooled_run(e, 65),
}


@pytest.mark.parametrize("site", sorted(STALE))
def test_planes_are_rewritten_every_call(ext, site):
    run, sizes = STALE[site](ext)
    first = [t.clone() for t in run(*fresh(sizes))[:len(sizes)]]
    torch.cuda.synchronize()
    ws = ext.det_workspace()
    assert len(ws) >= 1
    for t in ws:
        assert t.dtype == torch.float32 and t.is_cuda
        t.fill_(float("nan"))
    again = run(*fresh(sizes))[:len(sizes)]
    torch.cuda.synchronize()
    for a, b in zip(first, again):
        assert bool(torch.isfinite(b).all())
        assert torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------
def _refused_calls(ext):
    B = 8
    g = torch.Generator(device="cuda").manual_seed(8)
    dy = torch.randn((B, 64), device="cuda", generator=g).to(bf16)
    dyp = torch.randn((B, 7, 7, 64), device="cuda", generator=g).to(bf16)
    am = p2.draw_am((B, 7, 7, 64), g)
    w = (torch.randn((KP, 64), device="cuda", generator=g) * 0.05).to(bf16)
    x1, dyp1, am1 = c1.dw_inputs(3, "random", 5)
    return {
        "mask_db": lambda: ext.mask_db(dy, dy, True, 0.5,
                                       torch.zeros(64, device="cuda")),
        "pool_scatter": lambda: ext.pool_scatter(
            dyp, dyp, am, torch.zeros(64, device="cuda"), 14, 14),
        "linear_dx_unpool": lambda: ext.linear_dx_unpool(
            dy, w, am, torch.zeros(64, device="cuda"), 7, 7, 64),
        "conv1_dw_pooled": lambda: ext.conv1_dw_pooled(
            x1, dyp1, am1, torch.zeros(800, device="cuda"),
            torch.zeros(32, device="cuda")),
    }


@pytest.mark.parametrize("op", ["mask_db", "pool_scatter", "linear_dx_unpool",
                                "conv1_dw_pooled"])
def test_uncovered_routes_raise(ext, monkeypatch, op):
    if op == "conv1_dw_pooled":
        monkeypatch.setenv("DMNIST_CONV1_VALU", "1")
    call = _refused_calls(ext)[op]
    with pytest.raises(RuntimeError, match=op):
        call()
    ext.set_deterministic(False)
    assert ext.get_deterministic() is False
    call()                      # behaves as before with the switch off
    torch.cuda.synchronize()


def _flags(tag, *extra):
    from distributedmnist_amd.utils.flags import build_train_parser
    return build_train_parser().parse_args(
        ["--synthetic_data", "--train_dir", f"/tmp/dmdet_{tag}",
         "--model", "lenet", "--save_interval_secs", "100000", *extra])


def test_trainer_refuses_mlp_on_gpu(ext):
    from distributedmnist_amd.engine.train import Trainer
    flags = _flags("mlp", "--deterministic", "--batch_size", "32",
                   "--model", "mlp")
    with pytest.raises(ValueError, match="--model mlp"):
        Trainer(flags, device=torch.device("cuda:0"))
    Trainer(_flags("mlp0", "--batch_size", "32", "--model", "mlp"),
            device=torch.device("cuda:0"))
    assert ext.get_deterministic() is False


# ---------------------------------------------------------------------------
# 9. one step, graph against eager
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", ["0", "2"])
def test_step_graph_equals_eager(ext, monkeypatch, overlap):
    from distributedmnist_amd.engine.fused_step import FusedLeNetStep
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    monkeypatch.setenv("DMNIST_OVERLAP", overlap)
    B = 128
    flags = _flags(f"step{overlap}", "--deterministic", "--batch_size",
                   str(B), "--max_steps", "1", "--hip_graph", "off")
    t = Trainer(flags, device=torch.device("cuda:0"))
    assert ext.get_deterministic() is True
    ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
    x, y = ds.next_batch(B)
    step = FusedLeNetStep(t)
    step.overlap_allreduce = False
    assert step.overlap_level == int(overlap)
    step_dev = torch.zeros(1, dtype=torch.int64, device=t.device)
    fp = t.fp
    fp.flat_grad.zero_()
    loss_e, acc_e = step(x, y, step_dev)      # eager (and the warm-up)
    torch.cuda.synchronize()
    grad_e = fp.flat_grad.clone()
    loss_e, acc_e = loss_e.clone(), acc_e.clone()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            loss_g, acc_g = step(x, y, step_dev)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        fp.flat_grad.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(fp.flat_grad), bits(grad_e))
        assert torch.equal(loss_g, loss_e) and torch.equal(acc_g, acc_e)
    assert bool((grad_e != 0).any())


# ---------------------------------------------------------------------------
# 10. training runs
# ---------------------------------------------------------------------------
def _train(graph, tag, B, steps):
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    argv = ["--deterministic", "--batch_size", str(B), "--max_steps",
            str(steps), "--initial_learning_rate", "0.05", "--momentum",
            "0.9", "--moving_average_decay", "0.99", "--drop_connect"]
    if not graph:
        argv += ["--hip_graph", "off"]
    flags = _flags(tag, *argv)
    t = Trainer(flags, device=torch.device("cuda:0"))
    ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
    losses = []
    for _ in range(steps):
        x, y = ds.next_batch(B)
        _, loss, _, _ = t.graph_or_eager_step(x, y)
        losses.append(float(loss))
    torch.cuda.synchronize()
    if graph:
        assert t._graph is not None, "graph capture failed on GPU"
    return t.fp.flat_master.cpu(), t.flat_ema.cpu(), losses


@pytest.mark.parametrize("graph,B,steps", [(True, 192, 8), (False, 192, 8),
                                           (True, 4096, 3)])
def test_training_runs_are_bitwise_repeatable(ext, graph, B, steps):
    w1, e1, l1 = _train(graph, f"r1_{int(graph)}_{B}", B, steps)
    w2, e2, l2 = _train(graph, f"r2_{int(graph)}_{B}", B, steps)
    assert l1 == l2, (l1, l2)
    assert torch.equal(bits(w1), bits(w2))
    assert torch.equal(bits(e1), bits(e2))
    assert len(set(l1)) > 1
