"""--optimizer muon on the GPU: muon_orthogonalize on both routes against the
float64 replay of test_muon_cpu, muon_step against ops/cpu_ref.py, and
trainer runs, eager and graphed (docs/KERNELS.md "Muon").

Tolerance of the orthogonalisation: 3 times the error of
cpu_ref.muon_orthogonalize against the same float64 replay on the same input.
The factor covers the different summation order of the fp32 accumulations
and nothing more: a wrong tile, a dropped tail or a missing mirror moves the
error to order 1."""

import pytest
import torch
from test_muon_cpu import gaussian, rel_err, replay

from distributedmnist_amd.ops import cpu_ref
from distributedmnist_amd.ops import functional as Fx

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CASES = [("lds", (25, 32)), ("lds", (512, 10)), ("lds", (800, 64)),
         ("lds", (40, 16)),
         # a row tail, two column tiles and one mirrored off-diagonal tile;
         # rows < cols; a single tile with a K tail
         ("tiled", (200, 128)), ("tiled", (136, 256)), ("tiled", (72, 64)),
         ("auto", (200, 128)), ("auto", (40, 16))]


@pytest.mark.parametrize("iters", [1, 5])
@pytest.mark.parametrize("route,shape", CASES, ids=[
    f"{r}-{s[0]}x{s[1]}" for r, s in CASES])
def test_orthogonalize_against_float64(route, shape, iters):
    x = gaussian(shape)
    want = replay(x, iters)
    ref_err = rel_err(cpu_ref.muon_orthogonalize(x, iters), want)
    got = Fx.muon_orthogonalize(x.to(DEV), iters, route)
    assert got.dtype == torch.bfloat16 and got.shape == x.shape
    err = rel_err(got.cpu(), want)
    print(f"muon {route} {shape} iters={iters}: err {err:.5f}, "
          f"cpu_ref {ref_err:.5f}")
    assert err <= 3 * ref_err
    again = Fx.muon_orthogonalize(x.bfloat16().to(DEV), iters, route)
    assert torch.equal(got, again)


@pytest.mark.parametrize("route,shape", [("lds", (800, 128)),
                                         ("lds", (2000, 64)),
                                         ("tiled", (64, 96)),
                                         ("tiled", (60, 64)),
                                         ("auto", (64, 96))])
def test_impossible_route_is_an_error(route, shape):
    with pytest.raises(RuntimeError, match="fits"):
        Fx.muon_orthogonalize(torch.ones(shape, device=DEV), 5, route)


LENET = [(25, 32), (32,), (800, 64), (64,), (3136, 512), (512,), (512, 10),
         (10,)]
LR, MU, WD, D = 0.02, 0.9, 0.01, 0.9


def grow(bound, u, w0, offsets, numels, lr):
    """One update's share of the weight tensors' bound, from the update u."""
    bound *= 1 - lr * WD
    for o, m, s in zip(offsets, numels, LENET):
        if len(s) > 1:
            x = u[o:o + m].view(-1, s[-1])
            want = replay(x, 5)
            e = (cpu_ref.muon_orthogonalize(x).double() - want).abs().max()
            bound[o:o + m] += (3 * float(e) * lr * cpu_ref.muon_scale(*x.shape)
                               + 2.0 ** -23 * w0[o:o + m].abs().double())


@pytest.mark.parametrize("ema", [False, True], ids=["noema", "ema"])
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
def test_step_against_cpu_ref(ema, clip):
    """Two consecutive updates of LeNet's eight tensors.  The momentum buffer
    and the biases are elementwise: bit-exact.  A weight tensor may differ by
    the orthogonalisation's bound (3 times cpu_ref's own error against
    float64, as above) times the step lr * 0.2*sqrt(max(rows, cols)), plus
    one fp32 ulp of |w|, per update."""
    gen = torch.Generator().manual_seed(7)
    numels = [int(torch.Size(s).numel()) for s in LENET]
    offsets = [sum(numels[:i]) for i in range(len(numels))]
    cols = [s[-1] for s in LENET]
    adapt = sum(1 << i for i, s in enumerate(LENET) if len(s) > 1)
    n = sum(numels)
    state = dict(master=torch.randn(n, generator=gen) * 0.1,
                 mom=torch.zeros(n), ema=torch.randn(n, generator=gen))
    dev = {k: v.to(DEV) for k, v in state.items()}
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    coef = torch.tensor([0.5]) if clip else None
    kw = dict(offsets=offsets, numels=numels, cols=cols, adapt_mask=adapt)
    bound = torch.zeros(n, dtype=torch.float64)
    for k in range(2):
        g = 2 * torch.randn(n, generator=gen)
        gd = g.to(DEV)
        w0 = state["master"].clone()
        cpu_ref.muon_step(state["master"], g, state["mom"], LR, 0.5, MU, WD,
                          ema=state["ema"] if ema else None, ema_decay=D,
                          offset=k, clip_coef=coef, **kw)
        Fx.muon_step(dev["master"], gd, dev["mom"], LR, 0.5, MU, WD,
                     shadow=shadow, ema=dev["ema"] if ema else None,
                     ema_decay=D, offset=k,
                     clip_coef=coef.to(DEV) if clip else None, zero_grad=True,
                     **kw)
        assert not bool(gd.any())
        assert torch.equal(dev["mom"].cpu(), state["mom"])
        u = (g * 0.5) * (0.5 if clip else 1.0)
        u = u + state["mom"] * cpu_ref._f32(MU)
        grow(bound, u, w0, offsets, numels, LR)
        diff = (dev["master"].cpu().double() - state["master"].double()).abs()
        print(f"muon_step update {k}: max diff {float(diff.max()):.3e}, "
              f"max bound {float(bound.max()):.3e}")
        assert bool((diff <= bound).all())
        for o, m, s in zip(offsets, numels, LENET):
            if len(s) == 1:
                assert bool((diff[o:o + m] == 0).all()), s
        assert torch.equal(shadow, dev["master"].bfloat16())
    if ema:
        # the average moves towards the master: it inherits its bound
        e = (dev["ema"].cpu().double() - state["ema"].double()).abs()
        assert bool((e <= 1.001 * bound + 2.0 ** -22 * state["ema"].abs()).all())


B, STEPS = 64, 3


def trainer_run(tmp_path, tag, device, steps=STEPS, *extra):
    from distributedmnist_amd import _C
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    if "--device_data" not in extra:
        extra += ("--synthetic_data",)
    flags = build_train_parser().parse_args(
        ["--model", "lenet", "--batch_size", str(B),
         "--optimizer", "muon", "--momentum", "0.95", "--weight_decay",
         "0.01", "--save_interval_secs", "100000", "--train_dir",
         str(tmp_path / tag), *extra])
    try:
        t = Trainer(flags, device=torch.device(device))
        t.train(make_dataset(flags, 0, 1, t.device, t.compute_dtype),
                max_steps=steps)
        if device != "cpu":
            torch.cuda.synchronize()
        return t
    finally:
        if device != "cpu":
            _C.ext().set_deterministic(False)


def test_trainer_eager_graph_and_resume_agree_bitwise(tmp_path):
    """Compared under --deterministic: without it the backward kernels add
    the gradients with fp32 atomics and two runs of one scope differ."""
    eager = trainer_run(tmp_path, "e1", "cuda:0", STEPS, "--deterministic",
                        "--hip_graph", "off")
    graph = trainer_run(tmp_path, "g", "cuda:0", STEPS, "--deterministic")
    again = trainer_run(tmp_path, "e2", "cuda:0", STEPS, "--deterministic",
                        "--hip_graph", "off")
    assert graph._graph is not None and eager._graph is None
    assert bool(eager.flat_momentum.any())
    for t in (graph, again):
        assert torch.equal(t.fp.flat_master, eager.fp.flat_master)
        assert torch.equal(t.flat_momentum, eager.flat_momentum)
    # a checkpoint after step 2, resumed, reproduces step 3.  The synthetic
    # stream restarts with the process, so these runs draw from the resident
    # set, whose batches are a function of the step.
    from distributedmnist_amd.data.mnist_data import write_random_idx
    write_random_idx(str(tmp_path / "data"), 256, 150, seed=2)
    data = ("--deterministic", "--hip_graph", "off", "--device_data",
            "--data_dir", str(tmp_path / "data"))
    straight = trainer_run(tmp_path, "s", "cuda:0", STEPS, *data)
    trainer_run(tmp_path, "r", "cuda:0", 2, *data)
    resumed = trainer_run(tmp_path, "r", "cuda:0", STEPS, *data)
    assert resumed.step == STEPS
    assert torch.equal(resumed.fp.flat_master, straight.fp.flat_master)
    assert torch.equal(resumed.flat_momentum, straight.flat_momentum)


def test_cpu_trainer_follows_the_gpu_trainer(tmp_path):
    """The CPU trainer's update call site against the GPU trainer's, three
    steps, within the bound of test_step_against_cpu_ref accumulated.  The two
    devices draw different dropout masks and compute in different precisions,
    so their own gradients are not comparable: the CPU trainer is fed the GPU
    trainer's aggregated bucket, which an eager step leaves in place."""
    from distributedmnist_amd.engine.train import make_dataset
    gpu = trainer_run(tmp_path, "g", "cuda:0", 0, "--hip_graph", "off")
    cpu = trainer_run(tmp_path, "c", "cpu", 0, "--device", "cpu")
    assert torch.equal(cpu.fp.flat_master, gpu.fp.flat_master.cpu())
    ds = make_dataset(gpu.flags, 0, 1, gpu.device, gpu.compute_dtype)
    fp, lr = cpu.fp, gpu.flags.initial_learning_rate
    bound = torch.zeros(fp.flat_master.numel(), dtype=torch.float64)
    for k in range(STEPS):
        assert gpu.train_step(*gpu.to_device(*ds.next_batch(B)))[0]
        g, w0 = gpu.fp.flat_grad.cpu(), fp.flat_master.clone()
        cpu._apply_update(g.clone(), 1)
        cpu.step += 1
        assert torch.equal(cpu.flat_momentum, gpu.flat_momentum.cpu())
        grow(bound, g + cpu.flat_momentum * cpu_ref._f32(0.95), w0,
             fp.offsets, fp.numels, lr)
        diff = (gpu.fp.flat_master.cpu().double() - fp.flat_master.double()).abs()
        print(f"muon trainers step {k}: max diff {float(diff.max()):.3e}, "
              f"max bound {float(bound.max()):.3e}")
        assert bool((diff <= bound).all())
