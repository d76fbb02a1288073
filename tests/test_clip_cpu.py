"""Global-norm gradient clipping (--clip_grad_norm), CPU side: flag parsing,
cpu_ref.grad_norm and the clipped sgd_step against
torch.nn.utils.clip_grad_norm_ + torch.optim.SGD, the trainer end to end and
two gloo ranks."""

import math

import pytest
import torch
from mp_utils import init_pg, spawn_collect

from distributedmnist_amd.ops import cpu_ref
from distributedmnist_amd.ops import functional as Fx

EPS = 2.0 ** -24


# -- flag -------------------------------------------------------------------------

def test_flag_parsing(capsys):
    from distributedmnist_amd.utils.flags import build_train_parser
    p = build_train_parser()
    assert p.parse_args([]).clip_grad_norm == 0.0
    assert p.parse_args(["--clip_grad_norm", "0.5"]).clip_grad_norm == 0.5
    assert p.parse_args(["--clip_grad_norm", "inf"]).clip_grad_norm == math.inf
    assert p.parse_args(["--clip_grad_norm", "0"]).clip_grad_norm == 0.0
    for bad in ("-1", "nan", "abc", "-inf"):
        with pytest.raises(SystemExit) as ei:
            p.parse_args(["--clip_grad_norm", bad])
        assert ei.value.code == 2
    assert "--clip_grad_norm" in capsys.readouterr().err


# -- cpu_ref.grad_norm against torch ------------------------------------------------

def lenet_with_grads(seed):
    """A LeNet on flat buffers whose eight .grad views hold seeded values."""
    from distributedmnist_amd.models import build_model
    from distributedmnist_amd.parallel import FlatParams
    model = build_model("lenet", seed=66478, compute_dtype=torch.float32)
    fp = FlatParams(model, device="cpu", compute_dtype=torch.float32)
    g = torch.Generator().manual_seed(seed)
    for p in fp.params:
        p.grad.copy_(torch.randn(p.shape, generator=g))
    return model, fp


def test_grad_norm_matches_clip_grad_norm_():
    """cpu_ref.grad_norm + sgd_step(clip_coef=...) against
    torch.nn.utils.clip_grad_norm_ + torch.optim.SGD(momentum).

    The bounds (coefficient 4 * 2^-24 relative, masters
    4 * 2^-24 * max|w|, tests/test_ema_cpu.py::ema_atol(1, .)) are asserted
    against the two torch functions run on float64 copies of the eight
    parameters and gradients.  Run on the fp32 .grad views themselves, torch's
    own norm is not that accurate: on the 1,638,400-element fc1_w its fp32
    vector norm is low by about 400 * 2^-24 relative (measured against the
    float64 value when this test was written, torch 2.10 CPU, 8 threads), far
    outside the bound for any correct implementation.  The fp32 path is
    checked too, with the reference's own measured error (its fp32 against
    its fp64 coefficient) added to the same bounds."""
    model, fp = lenet_with_grads(11)
    assert len(fp.names) == 8 and fp.total == 1_663_370
    telemetry = cpu_ref.grad_norm(fp.flat_grad, fp.offsets, fp.numels, 1.0,
                                  math.inf)
    assert telemetry.dtype == torch.float32 and telemetry.shape == (10,)
    assert float(telemetry[1]) == 1.0
    clip = float(telemetry[0]) / 2  # half the measured norm
    stats = cpu_ref.grad_norm(fp.flat_grad, fp.offsets, fp.numels, 1.0, clip)
    assert torch.equal(stats[2:], telemetry[2:]) and stats[0] == telemetry[0]
    coef = float(stats[1])
    assert coef < 1.0
    for i, p in enumerate(fp.params):
        want = float(p.grad.double().norm())
        assert abs(float(stats[2 + i]) - want) <= 2 * EPS * want
    # one clipped momentum step of ours
    mu, lr = 0.9, 0.01
    w0 = fp.flat_master.clone()
    grad0 = fp.flat_grad.clone()
    mine = w0.clone()
    v = torch.zeros_like(mine)
    Fx.sgd_step(mine, grad0, lr, momentum=v, mu=mu, clip_coef=stats[1:2])
    assert torch.equal(fp.flat_grad, grad0)  # the gradient is left alone
    assert not torch.equal(mine, w0)
    wmax = float(w0.abs().max())
    tol = 4 * 1 * EPS * wmax  # ema_atol(1, [w])

    # the two torch functions in float64
    p64 = [p.detach().double().clone().requires_grad_() for p in fp.params]
    for q, p in zip(p64, fp.params):
        q.grad = p.grad.double().clone()
    total64 = float(torch.nn.utils.clip_grad_norm_(p64, clip))
    coef64 = min(1.0, clip / (total64 + 1e-6))
    torch.optim.SGD(p64, lr=lr, momentum=mu).step()
    w64 = torch.cat([q.detach().reshape(-1) for q in p64])
    err64 = float((mine.double() - w64).abs().max())
    print(f"fp64 reference: norm {float(stats[0])!r} / {total64!r}, coef "
          f"{coef!r} / {coef64!r} ({abs(coef - coef64) / coef64 / EPS:.2f} "
          f"x 2^-24), |master - torch| {err64:.3e} tol {tol:.3e}")
    assert abs(coef - coef64) <= 4 * EPS * coef64
    assert err64 <= tol

    # the same on the fp32 .grad views, the reference's own error added
    total32 = float(torch.nn.utils.clip_grad_norm_(fp.params, clip))
    coef32 = min(1.0, clip / (total32 + 1e-6))
    ref_err = abs(coef32 - coef64) / coef64
    torch.optim.SGD(fp.params, lr=lr, momentum=mu).step()
    err32 = float((mine.double() - fp.flat_master.double()).abs().max())
    tol32 = tol + lr * ref_err * coef64 * float(grad0.abs().max())
    print(f"fp32 reference: coef {coef32!r}, its own error "
          f"{ref_err / EPS:.1f} x 2^-24; |master - torch| {err32:.3e} tol "
          f"{tol32:.3e}")
    assert abs(coef - coef32) <= (4 * EPS + ref_err) * coef32
    assert err32 <= tol32


def test_grad_norm_scale_zero_and_bad_tables():
    g = torch.tensor([3.0, 4.0, 0.0, 12.0])
    s = cpu_ref.grad_norm(g, [0, 2], [2, 2], 0.5, 1.0)
    assert s.tolist()[0] == 6.5 and s.tolist()[2:] == [2.5, 6.0]
    assert abs(float(s[1]) - 1.0 / (6.5 + 1e-6)) <= 2 * EPS
    z = cpu_ref.grad_norm(torch.zeros(5), [0], [5], 1.0, 0.25)
    assert z.tolist() == [0.0, 1.0, 0.0]
    for offs, lens in (([0, 3], [2, 2]), ([0, 2], [2, 1]), ([1], [3]),
                       ([], [])):
        with pytest.raises(ValueError):
            cpu_ref.grad_norm(g, offs, lens, 1.0, 1.0)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            cpu_ref.grad_norm(g, [0], [4], 1.0, bad)


def test_clip_coef_comes_before_mask_and_momentum():
    n = 260
    g = torch.Generator().manual_seed(5)
    w, grad = torch.randn(n, generator=g), torch.randn(n, generator=g)
    coef = torch.tensor([0.25])
    a, b = w.clone(), w.clone()
    va, vb = torch.full((n,), 0.5), torch.full((n,), 0.5)
    Fx.sgd_step(a, grad, 0.5, drop_connect_keep=0.9, seed=3, offset=5,
                momentum=va, mu=0.5, clip_coef=coef)
    Fx.sgd_step(b, grad * 0.25, 0.5, drop_connect_keep=0.9, seed=3, offset=5,
                momentum=vb, mu=0.5)
    assert torch.equal(a, b) and torch.equal(va, vb)


# -- trainer ----------------------------------------------------------------------

def run_trainer(tmp_path, tag, *extra, steps=3):
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    flags = build_train_parser().parse_args(
        ["--synthetic_data", "--train_dir", str(tmp_path / tag), "--device",
         "cpu", "--batch_size", "32", "--save_interval_secs", "100000",
         *extra])
    t = Trainer(flags)
    ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
    masters, norms = [t.fp.flat_master.clone()], []
    for _ in range(steps):
        x, y = t.to_device(*ds.next_batch(32))
        applied, *_ = t.train_step(x, y)
        assert applied
        masters.append(t.fp.flat_master.clone())
        if t.clip_stats is not None:
            norms.append(t.grad_norms())
    return t, masters, norms


@pytest.fixture(scope="module")
def telemetry_run(tmp_path_factory):
    return run_trainer(tmp_path_factory.mktemp("clip"), "inf",
                       "--clip_grad_norm", "inf")


def test_trainer_inf_is_the_flag_off_run(tmp_path, telemetry_run):
    t, masters, norms = telemetry_run
    off, masters_off, _ = run_trainer(tmp_path, "off")
    assert off.clip_stats is None and off.clipped_steps is None
    with pytest.raises(RuntimeError, match="clip_grad_norm"):
        off.grad_norms()
    for a, b in zip(masters, masters_off):
        assert torch.equal(a, b)
    assert not torch.equal(masters[0], masters[-1])
    assert int(t.clipped_steps) == 0 and t.clip_updates == 3
    assert t.clip_stats.dtype == torch.float32
    assert t.clip_stats.numel() == 2 + len(t.fp.names)
    assert t.clipped_steps.dtype == torch.int64
    for d in norms:
        assert set(d) == set(t.fp.names) | {"global", "clip_coef"}
        assert d["clip_coef"] == 1.0
        assert all(math.isfinite(v) and v > 0 for v in d.values())
        rss = math.sqrt(sum(d[k] ** 2 for k in t.fp.names))
        assert abs(rss - d["global"]) <= 1e-5 * d["global"]
    assert "flat_master" in t.checkpoint_payload()
    assert not any("clip" in k for k in t.checkpoint_payload())


@pytest.mark.parametrize("extra", [(), ("--model", "mlp")],
                         ids=["lenet", "mlp"])
def test_trainer_clips_to_the_threshold(tmp_path, telemetry_run, extra):
    if extra:
        _, _, norms = run_trainer(tmp_path, "inf", "--clip_grad_norm", "inf",
                                  *extra, steps=1)
    else:
        _, _, norms = telemetry_run
    clip = norms[0]["global"] / 2
    t, masters, clipped = run_trainer(tmp_path, "half", "--clip_grad_norm",
                                      repr(clip), *extra)
    assert int(t.clipped_steps) >= 1
    assert clipped[0]["global"] == norms[0]["global"]  # same first gradient
    want = clip / (norms[0]["global"] + 1e-6)
    assert abs(clipped[0]["clip_coef"] - want) <= 4 * EPS * want
    lr = t.flags.initial_learning_rate
    length = float((masters[1].double() - masters[0].double()).norm())
    print(f"clip {clip!r}: first update length {length!r}, lr*clip "
          f"{lr * clip!r}")
    assert abs(length - lr * clip) <= 1e-5 * lr * clip


def test_trainer_refuses_a_bad_threshold(tmp_path):
    from distributedmnist_amd.engine.train import Trainer
    from distributedmnist_amd.utils.flags import build_train_parser
    flags = build_train_parser().parse_args(
        ["--synthetic_data", "--train_dir", str(tmp_path / "td"),
         "--device", "cpu", "--model", "mlp"])
    for bad in (-1.0, float("nan")):
        flags.clip_grad_norm = bad
        with pytest.raises(ValueError, match="clip_grad_norm"):
            Trainer(flags)


def test_train_logs_the_clipped_count(tmp_path, caplog):
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    flags = build_train_parser().parse_args(
        ["--synthetic_data", "--train_dir", str(tmp_path / "td"), "--device",
         "cpu", "--model", "mlp", "--batch_size", "32", "--max_steps", "3",
         "--save_interval_secs", "100000", "--clip_grad_norm", "1e-3"])
    t = Trainer(flags)
    with caplog.at_level("INFO", logger="dmnist.train"):
        t.train(make_dataset(flags, 0, 1, t.device, t.compute_dtype))
    lines = [r.getMessage() for r in caplog.records
             if "updates clipped" in r.getMessage()]
    assert lines == ["Gradient clipping (--clip_grad_norm 0.001): 3 of 3 "
                     "updates clipped"]
    # the per-step line is a scraper contract: unchanged
    steps = [r.getMessage() for r in caplog.records
             if ": step " in r.getMessage()]
    assert len(steps) == 3 and all("clip" not in s.lower() for s in steps)


# -- two gloo ranks ---------------------------------------------------------------------

def _rank_train(rank, world, port, train_dir, extra, q):
    import torch.distributed as dist
    init_pg(rank, world, port)
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    flags = build_train_parser().parse_args(
        ["--synthetic_data", "--train_dir", train_dir,
         "--batch_size", "16", "--max_steps", "4", "--model", "mlp",
         "--device", "cpu", "--save_interval_secs", "100000",
         "--clip_grad_norm", "0.05"] + list(extra))
    t = Trainer(flags, rank=rank, world=world, local_rank=rank)
    t.train(make_dataset(flags, rank, world, t.device, t.compute_dtype))
    q.put((rank, t.fp.flat_master.numpy().tobytes(),
           t.clip_stats.numpy().tobytes(), int(t.clipped_steps),
           t.clip_stats.tolist()))
    dist.destroy_process_group()


@pytest.mark.timeout(240)
@pytest.mark.parametrize("extra", [
    (), ("--interval_method", "--interval_ms", "0")],
    ids=["full_sync", "interval"])
def test_world2_ranks_agree(tmp_path, extra):
    out = spawn_collect(_rank_train, 2, args=(str(tmp_path / "td"), extra))
    (w0, s0, c0, l0), (w1, s1, c1, l1) = out[0], out[1]
    assert w0 == w1
    assert s0 == s1
    assert c0 == c1 and c0 >= 1
    assert l0[0] > 0 and l0[1] < 1.0
