"""--optimizer muon on the CPU: ops/cpu_ref.py::muon_orthogonalize against a
float64 replay of the same recurrence without rounding, the flags, and a
trainer run (docs/KERNELS.md "Muon").  Inputs are seeded Gaussian matrices
rounded to bf16: Newton-Schulz amplifies rounding noise along near-zero
singular values, so rank-deficient inputs say nothing about an
implementation."""

import pytest
import torch

from distributedmnist_amd.ops import cpu_ref
from distributedmnist_amd.utils.flags import build_train_parser

# max |cpu_ref - float64| / max |float64| as measured when the rounding points
# were fixed (docs/KERNELS.md); the test allows twice that
MEASURED = {((25, 32), 1): 0.00317, ((25, 32), 5): 0.01125,
            ((512, 10), 1): 0.00272, ((512, 10), 5): 0.02117,
            ((200, 128), 1): 0.00220, ((200, 128), 5): 0.01980}


def gaussian(shape):
    g = torch.Generator().manual_seed(shape[0] * 1000 + shape[1])
    return torch.randn(shape, generator=g).bfloat16().float()


def replay(x, iters):
    """The recurrence in float64, nothing rounded."""
    a, b, c = cpu_ref.MUON_ABC
    X = x.double()
    X = X / (X.norm() + 1e-7)
    for _ in range(iters):
        G = X.t() @ X
        X = a * X + X @ (b * G + c * (G @ G))
    return X


def rel_err(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("shape,iters", sorted(MEASURED))
def test_orthogonalize_against_float64(shape, iters):
    x = gaussian(shape)
    got = cpu_ref.muon_orthogonalize(x, iters)
    assert got.dtype == torch.bfloat16 and got.shape == x.shape
    err = rel_err(got, replay(x, iters))
    print(f"muon cpu_ref {shape} iters={iters}: err {err:.5f}")
    assert err <= 2 * MEASURED[shape, iters]
    if iters == 5:
        sv = torch.linalg.svdvals(got.double())
        assert 0.6 <= float(sv.min()) and float(sv.max()) <= 1.2, sv


@pytest.mark.parametrize("argv,ok", [
    (["--lars_eta", "0.01"], False),
    (["--adam_beta1", "0.9"], False),
    (["--weight_decay", "0.01", "--momentum", "0.95"], True)])
def test_flags(argv, ok, capsys):
    parser = build_train_parser()
    if ok:
        ns = parser.parse_args(["--optimizer", "muon", *argv])
        assert (ns.optimizer, ns.momentum, ns.weight_decay) == (
            "muon", 0.95, 0.01)
    else:
        with pytest.raises(SystemExit):
            parser.parse_args(["--optimizer", "muon", *argv])
        assert "argument " + argv[0] in capsys.readouterr().err


def cpu_trainer(tmp_path, tag, steps, *extra):
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    flags = build_train_parser().parse_args(
        ["--synthetic_data", "--device", "cpu", "--model", "mlp",
         "--batch_size", "64", "--optimizer", "muon", "--momentum", "0.95",
         "--weight_decay", "0.01", "--save_interval_secs", "100000",
         "--train_dir", str(tmp_path / tag), *extra])
    t = Trainer(flags)
    ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
    losses = []
    for _ in range(steps):
        applied, loss, _, _ = t.train_step(*t.to_device(*ds.next_batch(64)))
        assert applied
        losses.append(float(loss))
    return t, losses


def test_trainer_learns_and_checkpoints_momentum(tmp_path):
    t, losses = cpu_trainer(tmp_path, "learn", 30)
    assert losses[-1] < losses[0], losses
    payload = t.checkpoint_payload()
    assert torch.equal(payload["flat_momentum"], t.flat_momentum)
    assert bool(t.flat_momentum.any())
    assert not any("muon" in k for k in payload)
    # mu = 0 is legal: an orthogonalised gradient
    t0, _ = cpu_trainer(tmp_path, "mu0", 1, "--momentum", "0")
    assert torch.equal(t0.flat_momentum, t0.fp.flat_grad)
