"""Weight moving average on the GPU: sgd_step_kernel_ema against the CPU
reference, ema_publish_kernel against sync_shadow(), the graphed and the
eager trainer against a replay of their own masters, and in-training
evaluation on the twin."""

import pytest
import torch

from distributedmnist_amd.data.mnist_data import write_random_idx
from distributedmnist_amd.ops import functional as Fx

pytestmark = pytest.mark.gpu

D = 0.5
# powers of two: lr*g and mu*v are exact, so the fused multiply-adds of the
# kernel and the separate multiply + add of the CPU reference round the same
# values and the masters agree bit for bit; what is left in the average is
# its own arithmetic
LR, MU = 0.125, 0.5
PAD = 8  # canary elements past n


@pytest.fixture(scope="module")
def ext():
    from distributedmnist_amd import _C
    return _C.ext()


def bits(x):
    return x.view(torch.int16).cpu()


def decay_at(decay, k):
    return min(decay, (1.0 + k) / (10.0 + k))


def replay(e0, masters, decay, k0=1):
    e = e0.double().cpu().clone()
    for i, w in enumerate(masters):
        e = e - (1.0 - decay_at(decay, k0 + i)) * (e - w.double().cpu())
    return e


def ema_atol(n_updates, masters):
    """4 * n * 2^-24 * max|w| (tests/test_ema_cpu.py)."""
    return 4 * n_updates * 2.0 ** -24 * max(float(w.abs().max())
                                            for w in masters)


_inputs = {}


def inputs(n):
    """(master, three gradients) on the CPU, built once per size."""
    if n not in _inputs:
        g = torch.Generator().manual_seed(n)
        _inputs[n] = (torch.randn(n, generator=g),
                      [torch.randn(n, generator=g) for _ in range(3)])
    return _inputs[n]


_reference = {}


def cpu_reference(n, momentum, offset0):
    """Three updates through ops/cpu_ref.py, computed once per case:
    per-update (master, average)."""
    key = (n, momentum, offset0)
    if key not in _reference:
        w0, grads = inputs(n)
        m, e = w0.clone(), w0.clone()
        v = torch.zeros(n) if momentum else None
        out = []
        for i, g in enumerate(grads):
            Fx.sgd_step(m, g, LR, offset=offset0 + i, momentum=v,
                        mu=MU if momentum else 0.0, ema=e, ema_decay=D)
            out.append((m.clone(), e.clone()))
        _reference[key] = out
    return _reference[key]


def gpu_state(n, momentum):
    w0, _ = inputs(n)
    buf = torch.full((n + PAD,), 7.5, device="cuda")
    buf[:n] = w0.cuda()
    return dict(master=w0.cuda(), ema_buf=buf,
                shadow=torch.zeros(n, dtype=torch.bfloat16, device="cuda"),
                mom=torch.zeros(n, device="cuda") if momentum else None)


# 1, 3: a scalar tail alone; 4: one float4 group; 5, 1027: groups + a tail;
# 2_097_157 > 2048*256*4: the grid-stride loop takes a second trip
SIZES = [1, 3, 4, 5, 1027, 2_097_157]
# offsets 6, 7, 8 -> k = 7, 8, 9: both branches of min(D, (1+k)/(10+k))
OFFSET0 = 6


@pytest.mark.parametrize("by_device", [False, True], ids=["value", "dev"])
@pytest.mark.parametrize("momentum", [False, True], ids=["sgd", "momentum"])
@pytest.mark.parametrize("n", SIZES)
def test_sgd_step_with_average_matches_cpu_reference(ext, n, momentum,
                                                     by_device):
    _, grads = inputs(n)
    ref = cpu_reference(n, momentum, OFFSET0)
    on, off = gpu_state(n, momentum), gpu_state(n, momentum)
    mu = MU if momentum else 0.0
    lr_dev = torch.tensor([LR], device="cuda")
    masters = []
    for i, g in enumerate(grads):
        g_on, g_off = g.cuda(), g.cuda()
        ema = on["ema_buf"][:n]
        if by_device:
            # zero_grad on: the bucket is cleared in the same pass
            off_dev = torch.tensor([OFFSET0 + i], dtype=torch.int64,
                                   device="cuda")
            ext.sgd_step_dev(on["master"], g_on, on["shadow"], True, lr_dev,
                             -1.0, 0, off_dev, momentum=on["mom"], mu=mu,
                             zero_grad=True, ema=ema, ema_decay=D)
            ext.sgd_step_dev(off["master"], g_off, off["shadow"], True,
                             lr_dev, -1.0, 0, off_dev, momentum=off["mom"],
                             mu=mu, zero_grad=True)
            assert not g_on.any() and not g_off.any()
        else:
            ext.sgd_step(on["master"], g_on, on["shadow"], True, LR, 1.0,
                         -1.0, 0, OFFSET0 + i, momentum=on["mom"], mu=mu,
                         ema=ema, ema_decay=D)
            ext.sgd_step(off["master"], g_off, off["shadow"], True, LR, 1.0,
                         -1.0, 0, OFFSET0 + i, momentum=off["mom"], mu=mu)
            assert torch.equal(g_on, g.cuda())  # gradient left alone
        # everything but the average: the same bits as the pass without it
        assert torch.equal(on["master"], off["master"])
        assert torch.equal(bits(on["shadow"]), bits(off["shadow"]))
        assert torch.equal(g_on, g_off)
        if momentum:
            assert torch.equal(on["mom"], off["mom"])
        masters.append(on["master"].cpu())
        m_ref, e_ref = ref[i]
        tol = ema_atol(i + 1, [m for m, _ in ref[:i + 1]])
        err = float((ema.cpu().double() - e_ref.double()).abs().max())
        print(f"n={n} update {i + 1}: |ema - cpu_ref| {err:.3e} tol {tol:.3e}")
        assert err <= tol, (n, i, err, tol)
        assert torch.equal(on["master"].cpu(), m_ref)
        assert bool((on["ema_buf"][n:] == 7.5).all())  # canaries
    w0, _ = inputs(n)
    err = float((on["ema_buf"][:n].cpu().double()
                 - replay(w0, masters, D, k0=OFFSET0 + 1)).abs().max())
    assert err <= ema_atol(3, masters)


def test_sgd_step_average_with_drop_connect(ext):
    """The post-aggregation mask changes the master, not the rule."""
    n = 1027
    w0, grads = inputs(n)
    on, off = gpu_state(n, False), gpu_state(n, False)
    ema = on["ema_buf"][:n]
    ext.sgd_step(on["master"], grads[0].cuda(), on["shadow"], True, LR, 1.0,
                 0.9, 3, 5, ema=ema, ema_decay=D)
    ext.sgd_step(off["master"], grads[0].cuda(), off["shadow"], True, LR, 1.0,
                 0.9, 3, 5)
    assert torch.equal(on["master"], off["master"])
    m = on["master"].cpu()
    err = float((ema.cpu().double() - replay(w0, [m], D, k0=6)).abs().max())
    assert err <= ema_atol(1, [m])
    assert bool((on["ema_buf"][n:] == 7.5).all())


def test_sgd_step_refuses_bad_average_arguments(ext):
    m = torch.zeros(8, device="cuda")
    g = torch.zeros(8, device="cuda")
    sh = torch.zeros(8, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="shorter"):
        ext.sgd_step(m, g, sh, True, 0.1, 1.0, -1.0, 0, 0,
                     ema=torch.zeros(4, device="cuda"), ema_decay=D)
    with pytest.raises(RuntimeError, match="ema_decay"):
        ext.sgd_step(m, g, sh, True, 0.1, 1.0, -1.0, 0, 0,
                     ema=torch.zeros(8, device="cuda"), ema_decay=1.0)
    with pytest.raises(RuntimeError, match="fp32"):
        ext.sgd_step(m, g, sh, True, 0.1, 1.0, -1.0, 0, 0, ema=sh,
                     ema_decay=D)


# -- ema_publish ------------------------------------------------------------------

def build(model_name):
    from distributedmnist_amd.models import build_model
    from distributedmnist_amd.parallel import FlatParams
    model = build_model(model_name, seed=66478,
                        compute_dtype=torch.bfloat16).to("cuda")
    fp = FlatParams(model, device=torch.device("cuda"),
                    compute_dtype=torch.bfloat16)
    return model, fp


@pytest.mark.parametrize("model_name", ["lenet", "mlp"])
def test_ema_publish_equals_sync_shadow(model_name):
    model, fp = build(model_name)
    assert fp._t_pairs, "the layout under test has transposed weights"
    # row or column counts that are no multiple of 32 (fc2_w is K x 10)
    assert any(r % 32 or c % 32 for _, r, c in fp._t_slices)
    g = torch.Generator().manual_seed(3)
    fp.flat_master.copy_(torch.randn(fp.total, generator=g).cuda())
    fp.sync_shadow()
    want_flat = bits(fp.flat_shadow)
    want_t = [bits(t) for _, t in fp._t_pairs]
    fp.flat_shadow.fill_(-3.0)
    for _, t in fp._t_pairs:
        t.fill_(-3.0)
    master = fp.flat_master.clone()
    fp.publish()
    assert torch.equal(bits(fp.flat_shadow), want_flat)
    for (_, t), want in zip(fp._t_pairs, want_t):
        assert torch.equal(bits(t), want), tuple(t.shape)
    assert torch.equal(fp.flat_master, master)  # read only
    # the views the forward kernels hold are the buffers just written
    for n, t in model.shadows_T.items():
        v = model.shadows[n]
        assert torch.equal(bits(t), bits(v.reshape(-1, v.shape[-1]).t()
                                         .contiguous()))


def test_ema_publish_checks_its_slices(ext):
    e = torch.zeros(64, device="cuda")
    sh = torch.zeros(64, dtype=torch.bfloat16, device="cuda")
    dst = torch.zeros(8, 8, dtype=torch.bfloat16, device="cuda")
    ext.ema_publish(e, sh, [0], [8], [8], [dst])  # exactly fits
    with pytest.raises(RuntimeError, match="outside"):
        ext.ema_publish(e, sh, [1], [8], [8], [dst])
    with pytest.raises(RuntimeError, match="wrong size"):
        ext.ema_publish(e, sh, [0], [4], [8], [dst])
    with pytest.raises(RuntimeError, match="shadow size"):
        ext.ema_publish(e, sh[:32], [], [], [], [])


# -- trainer: graph and eager --------------------------------------------------------

def trainer_run(tmp_path, tag, *extra, steps=4):
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    flags = build_train_parser().parse_args(
        ["--synthetic_data", "--model", "lenet", "--batch_size", "64",
         "--train_dir", str(tmp_path / tag), "--moving_average_decay",
         str(D), "--save_interval_secs", "100000", *extra])
    t = Trainer(flags, device=torch.device("cuda:0"))
    ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
    w0 = t.fp.flat_master.clone()
    assert torch.equal(t.flat_ema, w0)
    masters = []
    for _ in range(steps):
        x, y = t.to_device(*ds.next_batch(64))
        applied, loss, _, _ = t.graph_or_eager_step(x, y)
        assert applied and float(loss) == float(loss)
        masters.append(t.fp.flat_master.clone())
    return t, w0, masters


@pytest.mark.parametrize("extra", [("--hip_graph", "off"), (),
                                   ("--momentum", "0.9")],
                         ids=["eager", "graph", "graph_momentum"])
def test_trainer_average_equals_replay_of_its_own_masters(tmp_path, extra):
    t, w0, masters = trainer_run(tmp_path, "td", *extra)
    if "off" in extra:
        assert t._graph is None
    else:
        assert t._graph is not None, "capture must engage"
    assert not torch.equal(masters[0], w0)
    want = replay(w0, masters, D)
    err = float((t.flat_ema.cpu().double() - want).abs().max())
    tol = ema_atol(4, masters)
    print(f"{extra}: |flat_ema - replay| {err:.3e} tol {tol:.3e}")
    # also: the three warm-up steps of the capture left no trace
    assert err <= tol


# -- trainer: evaluation on the twin ----------------------------------------------------

def test_in_training_evaluation_reads_the_published_twin(tmp_path, monkeypatch):
    from distributedmnist_amd.engine.device_eval import DeviceEvaluator
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    data_dir = str(tmp_path / "data")
    write_random_idx(data_dir, 256, 150, seed=2)
    # the case tests/test_ema_cpu.py verified: 27 of the 150 argmaxes differ
    # between the twin and the live model on the CPU
    flags = build_train_parser().parse_args(
        ["--data_dir", data_dir, "--train_dir", str(tmp_path / "td"),
         "--model", "mlp", "--batch_size", "64", "--max_steps", "6",
         "--save_interval_secs", "100000", "--device_data",
         "--moving_average_decay", "0.9", "--initial_learning_rate", "0.5",
         "--eval_every_steps", "3", "--eval_batch_size", "64"])
    t = Trainer(flags, device=torch.device("cuda:0"))
    hist = t.train(make_dataset(flags, 0, 1, t.device, t.compute_dtype))
    assert t.evaluator.model is t.ema_model
    assert [h[0] for h in t.eval_history] == [3, 6]
    ds = t.evaluator.ds
    # a fresh eager forward of the twin's published shadows
    monkeypatch.setenv("DMNIST_EVAL_GRAPH", "0")
    t.ema_fp.sync_shadow()  # torch ops; must equal what ema_publish wrote
    eager = DeviceEvaluator(t.ema_model, ds, 64, "cuda")
    assert eager.graph is None
    twin = eager.run()
    live = DeviceEvaluator(t.model, ds, 64, "cuda").run()
    assert twin.num_examples == 150
    assert t.test_acc == twin.precision == hist[-1][2]
    again = t.evaluate_now()  # ema_publish + the captured chunk graph
    assert torch.equal(again.confusion, twin.confusion)
    assert again.precision == twin.precision and again.loss == twin.loss
    x = torch.empty((150, 28, 28, 1), dtype=torch.bfloat16, device="cuda")
    y = torch.empty(150, dtype=torch.int64, device="cuda")
    ds.range_into(x, y, start=0)
    with torch.no_grad():
        lt = t.ema_model(x, train=False).float()
        ll = t.model(x, train=False).float()
    assert round(twin.precision * 150) == int((lt.argmax(1) == y).sum())
    differ = int((lt.argmax(1) != ll.argmax(1)).sum())
    print(f"argmaxes that differ between twin and live model: {differ}")
    assert differ >= 1
    assert not torch.equal(twin.confusion, live.confusion)
