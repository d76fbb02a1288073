"""LARS (--lars_eta, --weight_decay), CPU side: the flags, cpu_ref.lars_norm
against a direct float64 computation, and the trainer end to end."""

import math

import pytest
import torch

from distributedmnist_amd.ops import cpu_ref
from distributedmnist_amd.utils.flags import build_train_parser

EPS = 2.0 ** -24


@pytest.mark.parametrize("argv", [
    ["--weight_decay", "5e-4"], ["--lars_eta", "-1"], ["--lars_eta", "nan"],
    ["--lars_eta", "0.001", "--weight_decay", "-1"]])
def test_bad_flags_are_argument_errors(argv, capsys):
    with pytest.raises(SystemExit) as ei:
        build_train_parser().parse_args(argv)
    assert ei.value.code == 2
    assert argv[-2] in capsys.readouterr().err  # names the flag at fault


@pytest.mark.parametrize("clip", [0.0, 2.0])
def test_lars_norm_against_float64(clip):
    """The odd table: odd offsets, a 1-element and an empty tensor, one that
    is not adaptive, an all-zero one.  Float64 sums, then at most 8 fp32
    roundings per entry."""
    offs, lens = [0, 1, 4, 4, 15, 1000], [1, 3, 0, 11, 985, 27]
    g = torch.Generator().manual_seed(3)
    w, gr = torch.randn(1027, generator=g), torch.randn(1027, generator=g)
    gr[4:15] = 0.0
    scale, eta, wd, adapt = 1.0 / 3, 0.001, 5e-4, 0b111011
    tab, st, cs = cpu_ref.lars_norm(w, gr, offs, lens, adapt, scale, eta, wd,
                                    clip)
    assert tab.shape == (32,) and st.shape == (18,)
    assert (cs is None) == (clip == 0)
    norm = scale * math.sqrt(float((gr.double() ** 2).sum()))
    coef = min(1.0, clip / (norm + 1e-6)) if clip else 1.0
    assert coef < 1.0 or not clip
    for t, (o, m) in enumerate(zip(offs, lens)):
        wn = math.sqrt(float((w.double()[o:o + m] ** 2).sum()))
        gn = coef * scale * math.sqrt(float((gr.double()[o:o + m] ** 2).sum()))
        ad = bool((adapt >> t) & 1)
        ratio = eta * wn / (gn + wd * wn) if ad and wn > 0 and gn > 0 else 1.0
        want = (ratio * coef, ratio * wd / scale if ad else 0.0, wn, gn, ratio)
        got = tab[2 * t:2 * t + 2].tolist() + st[3 * t:3 * t + 3].tolist()
        for a, b in zip(got, want):
            assert abs(a - b) <= 8 * EPS * abs(b), (t, got, want)
    assert st[3 * 2 + 2] == 1.0 and st[3 * 3 + 2] == 1.0  # empty, zero grad
    assert tab[4] == tab[6] and tab[5] == 0.0  # not adaptive: (coef, 0)
    for bad in (dict(eta=0.0), dict(wd=-1.0), dict(grad_scale=0.0),
                dict(eta=math.nan)):
        kw = dict(grad_scale=1.0, eta=eta, wd=wd)
        kw.update(bad)
        with pytest.raises(ValueError):
            cpu_ref.lars_norm(w, gr, offs, lens, adapt, **kw)


def run_trainer(tmp_path, tag, *extra):
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    flags = build_train_parser().parse_args(
        ["--synthetic_data", "--train_dir", str(tmp_path / tag), "--device",
         "cpu", "--batch_size", "32", "--momentum", "0.9",
         "--save_interval_secs", "100000", *extra])
    t = Trainer(flags)
    ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
    for _ in range(3):
        assert t.train_step(*t.to_device(*ds.next_batch(32)))[0]
    return t


@pytest.mark.parametrize("extra", [(), ("--model", "mlp"),
                                   ("--clip_grad_norm", "0.5")],
                         ids=["lenet", "mlp", "clip"])
def test_trainer_with_lars(tmp_path, extra):
    lars = ("--lars_eta", "0.001", "--weight_decay", "5e-4")
    off = run_trainer(tmp_path, "off", *extra)
    a = run_trainer(tmp_path, "a", *extra, *lars)
    b = run_trainer(tmp_path, "b", *extra, *lars)
    assert torch.equal(a.fp.flat_master, b.fp.flat_master)  # repeatable
    assert not torch.equal(a.fp.flat_master, off.fp.flat_master)
    with pytest.raises(RuntimeError, match="lars_eta"):
        off.trust_ratios()
    ratios = a.trust_ratios()
    assert set(ratios) == set(a.fp.names)
    for p, name in zip(a.fp.params, a.fp.names):
        wn, gn, r = ratios[name]
        assert math.isfinite(r) and (r == 1.0) == (p.dim() == 1), (name, r)
        if p.dim() > 1:
            want = 0.001 * wn / (gn + 5e-4 * wn)
            assert abs(r - want) <= 8 * EPS * want
    if extra and extra[0] == "--clip_grad_norm":
        assert a.grad_norms()["clip_coef"] <= 1.0 and int(a.clipped_steps) >= 1
    assert not any("lars" in k for k in a.checkpoint_payload())
