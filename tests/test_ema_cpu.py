"""Weight moving average (--moving_average_decay), CPU side: the sgd_step
recurrence against an fp64 replay, the trainer end to end, checkpoint /
resume / restore without an average, the evaluator CLI's
--use_moving_average, in-training evaluation on the twin, two gloo ranks and
argument validation."""

import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from mp_utils import init_pg, spawn_collect

from distributedmnist_amd.data.mnist_data import write_random_idx
from distributedmnist_amd.ops import cpu_ref
from distributedmnist_amd.ops import functional as Fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def decay_at(D, k):
    """d_k of the k-th update (k = 1, 2, ...), in python floats (fp64)."""
    return min(D, (1.0 + k) / (10.0 + k))


def replay(e0, masters, D, k0=1):
    """Independent fp64 replay: e0 the initial average, masters[i] the
    master after update k0 + i."""
    e = e0.double().clone()
    for i, w in enumerate(masters):
        e = e - (1.0 - decay_at(D, k0 + i)) * (e - w.double())
    return e


def ema_atol(n_updates, masters):
    """4 * n * 2^-24 * max|w|: two fp32 roundings per update, doubled for
    fused-multiply-add contraction differences."""
    wmax = max(float(w.abs().max()) for w in masters)
    return 4 * n_updates * 2.0 ** -24 * wmax


# -- the recurrence ---------------------------------------------------------------

def test_decay_schedule_switches_where_expected():
    # (1 + k)/(10 + k) >= 0.5 first at k = 8; > 0.9 first at k = 81
    assert [decay_at(0.5, k) < 0.5 for k in range(1, 13)] == \
        [True] * 7 + [False] * 5
    assert decay_at(0.5, 7) == 8 / 17 and decay_at(0.5, 8) == 0.5
    assert all(decay_at(0.9, k) < 0.9 for k in range(1, 80))  # 81/90 at 80
    assert decay_at(0.9, 81) == 0.9
    # the fp32 weight the kernel and the reference use
    assert cpu_ref.ema_weight(0.5, 0) == float(
        np.float32(1) - np.float32(2) / np.float32(11))
    assert cpu_ref.ema_weight(0.5, 7) == 0.5


@pytest.mark.parametrize("D", [0.9, 0.5])
@pytest.mark.parametrize("mu", [0.0, 0.9])
def test_recurrence_against_fp64_replay(D, mu):
    n, updates = 1027, 12
    g = torch.Generator().manual_seed(7)
    master = torch.randn(n, generator=g)
    a = dict(master=master.clone(), mom=torch.zeros(n) if mu else None,
             shadow=torch.zeros(n, dtype=torch.bfloat16))
    b = dict(master=master.clone(), mom=torch.zeros(n) if mu else None,
             shadow=torch.zeros(n, dtype=torch.bfloat16))
    e = master.clone()
    e0 = e.clone()
    masters = []
    for step in range(updates):
        grad = torch.randn(n, generator=g)
        Fx.sgd_step(a["master"], grad, lr=0.1, grad_scale=0.5, offset=step,
                    shadow=a["shadow"], momentum=a["mom"], mu=mu,
                    ema=e, ema_decay=D)
        Fx.sgd_step(b["master"], grad, lr=0.1, grad_scale=0.5, offset=step,
                    shadow=b["shadow"], momentum=b["mom"], mu=mu)
        # the average changes nothing else
        assert torch.equal(a["master"], b["master"])
        assert torch.equal(a["shadow"], b["shadow"])
        if mu:
            assert torch.equal(a["mom"], b["mom"])
        masters.append(a["master"].clone())
        err = float((e.double() - replay(e0, masters, D)).abs().max())
        tol = ema_atol(len(masters), masters)
        assert err <= tol, (step, err, tol)
    assert e.dtype == torch.float32
    assert not torch.equal(e, a["master"])  # it is an average, not a copy


def test_recurrence_with_drop_connect_mask():
    n = 260
    g = torch.Generator().manual_seed(8)
    m1 = torch.randn(n, generator=g)
    m2, e = m1.clone(), m1.clone()
    e0 = e.clone()
    grad = torch.randn(n, generator=g)
    Fx.sgd_step(m1, grad, lr=1.0, drop_connect_keep=0.9, seed=3, offset=5,
                ema=e, ema_decay=0.5)
    Fx.sgd_step(m2, grad, lr=1.0, drop_connect_keep=0.9, seed=3, offset=5)
    assert torch.equal(m1, m2)
    err = float((e.double() - replay(e0, [m1], 0.5, k0=6)).abs().max())
    assert err <= ema_atol(1, [m1])


def test_sgd_step_refuses_a_bad_decay():
    m = torch.zeros(4)
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            Fx.sgd_step(m, torch.zeros(4), lr=0.1, ema=m.clone(),
                        ema_decay=bad)


# -- trainer ----------------------------------------------------------------------

def train_flags(tmp_path, tag, *extra):
    from distributedmnist_amd.utils.flags import build_train_parser
    return build_train_parser().parse_args(
        ["--data_dir", str(tmp_path / "data"),
         "--train_dir", str(tmp_path / tag), "--device", "cpu",
         "--model", "mlp", "--batch_size", "64",
         "--save_interval_secs", "100000", *extra])


def make_data(tmp_path):
    write_random_idx(str(tmp_path / "data"), 256, 150, seed=2)


def run_steps(flags, steps):
    """Drive train_step by hand; returns (trainer, initial master, masters
    after each step)."""
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    t = Trainer(flags)
    ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
    w0 = t.fp.flat_master.clone()
    masters = []
    for _ in range(steps):
        x, y = t.to_device(*ds.next_batch(flags.batch_size))
        applied, *_ = t.train_step(x, y)
        assert applied
        masters.append(t.fp.flat_master.clone())
    return t, w0, masters


@pytest.mark.parametrize("extra", [
    (), ("--momentum", "0.9"), ("--drop_connect",),
    ("--drop_connect", "--drop_connect_post"), ("--model", "lenet")],
    ids=["plain", "momentum", "dc_pre", "dc_post", "lenet"])
def test_trainer_average_equals_replay_of_its_masters(tmp_path, extra):
    make_data(tmp_path)
    flags = train_flags(tmp_path, "td", "--moving_average_decay", "0.5",
                        *extra)
    t, w0, masters = run_steps(flags, 6)
    assert t.flat_ema is t.ema_fp.flat_master and t.ema_decay == 0.5
    assert t.flat_ema.data_ptr() != t.fp.flat_master.data_ptr()
    err = float((t.flat_ema.double() - replay(w0, masters, 0.5)).abs().max())
    assert err <= ema_atol(6, masters), err
    assert not torch.equal(t.flat_ema, t.fp.flat_master)
    # the twin's parameters (biases included) are views of the average
    for name in t.ema_model.PARAM_ORDER:
        p = getattr(t.ema_model, name)
        o = t.ema_fp.offsets[t.ema_fp.names.index(name)]
        assert p.data_ptr() == t.flat_ema[o:].data_ptr()
    # and the training trajectory is the flag-off one
    off, _, masters_off = run_steps(train_flags(tmp_path, "td2", *extra), 6)
    assert off.flat_ema is None and off.ema_model is None
    assert torch.equal(masters_off[-1], masters[-1])


def test_interval_mode_keys_the_average_on_the_generation(tmp_path):
    make_data(tmp_path)
    flags = train_flags(tmp_path, "td", "--moving_average_decay", "0.5",
                        "--interval_method", "--interval_ms", "0",
                        "--max_steps", "5")
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    t = Trainer(flags)
    w0 = t.fp.flat_master.clone()
    seen = []
    orig = t._apply_update

    def recording(grad, contributors):
        orig(grad, contributors)
        seen.append((t.engine.generation, t.fp.flat_master.clone()))

    t._apply_update = recording
    t.train(make_dataset(flags, 0, 1, t.device, t.compute_dtype))
    assert seen and [g for g, _ in seen] == list(range(1, len(seen) + 1))
    masters = [w for _, w in seen]
    err = float((t.flat_ema.double() - replay(w0, masters, 0.5)).abs().max())
    assert err <= ema_atol(len(masters), masters)


def _train(tmp_path, tag, max_steps, *extra):
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    flags = train_flags(tmp_path, tag, "--device_data", *extra)
    t = Trainer(flags)
    t.train(make_dataset(flags, 0, 1, t.device, t.compute_dtype),
            max_steps=max_steps)
    return t


def test_checkpoint_and_resume(tmp_path):
    """The CPU path is deterministic: the resumed average is the
    uninterrupted one, exactly."""
    from distributedmnist_amd.engine.supervisor import Supervisor
    make_data(tmp_path)
    ema = ("--moving_average_decay", "0.5", "--momentum", "0.9")
    straight = _train(tmp_path, "straight", 6, *ema)
    part = _train(tmp_path, "resumed", 3, *ema)
    step, payload = Supervisor.restore(str(tmp_path / "resumed"))
    assert step == 3
    assert torch.equal(payload["flat_ema"], part.flat_ema)
    assert payload["flat_ema"].dtype == torch.float32
    assert not torch.equal(payload["flat_ema"], payload["flat_master"])
    resumed = _train(tmp_path, "resumed", 6, *ema)
    assert resumed.step == 6
    assert torch.equal(resumed.fp.flat_master, straight.fp.flat_master)
    assert torch.equal(resumed.flat_ema, straight.flat_ema)


def test_payload_without_the_flag_has_no_average(tmp_path):
    make_data(tmp_path)
    t = _train(tmp_path, "plain", 2)
    payload = t.checkpoint_payload()
    assert "flat_ema" in payload and payload["flat_ema"] is None


def test_restore_without_an_average_warns_once(tmp_path, caplog):
    make_data(tmp_path)
    _train(tmp_path, "td", 3)  # no --moving_average_decay
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    flags = train_flags(tmp_path, "td", "--device_data",
                        "--moving_average_decay", "0.5")
    t = Trainer(flags)
    restored = []
    orig = t.train_step

    def spy(*a, **k):
        if not restored:  # before the first resumed step
            restored.append((t.flat_ema.clone(), t.fp.flat_master.clone()))
        return orig(*a, **k)

    t.train_step = spy
    with caplog.at_level("WARNING", logger="dmnist.train"):
        t.train(make_dataset(flags, 0, 1, t.device, t.compute_dtype),
                max_steps=4)
    warnings = [r for r in caplog.records if r.levelname == "WARNING"
                and "moving" in r.getMessage()]
    assert len(warnings) == 1
    assert "--moving_average_decay" in warnings[0].getMessage()
    e, w = restored[0]
    assert torch.equal(e, w)
    assert t.step == 4 and not torch.equal(t.flat_ema, t.fp.flat_master)


# -- in-training evaluation reads the twin -------------------------------------------

# lr 0.5 over 6 steps: the average lags the live weights far enough that the
# two models disagree on rows of the 150-example stand-in test set
# (verified on the CPU when this test was written; asserted below)
EVAL_ARGS = ("--moving_average_decay", "0.9", "--initial_learning_rate", "0.5",
             "--eval_every_steps", "3", "--eval_batch_size", "64",
             "--max_steps", "6", "--save_results_period", "1")


def held_out_logits(model, ds):
    x = torch.empty((ds.num_examples, 28, 28, 1))
    y = torch.empty(ds.num_examples, dtype=torch.int64)
    ds.range_into(x, y, start=0)
    with torch.no_grad():
        return model(x, train=False), y


def test_in_training_evaluation_uses_the_average(tmp_path):
    from distributedmnist_amd.engine.device_eval import DeviceEvaluator
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    make_data(tmp_path)
    flags = train_flags(tmp_path, "td", *EVAL_ARGS)
    t = Trainer(flags)
    hist = t.train(make_dataset(flags, 0, 1, t.device, t.compute_dtype))
    assert t.evaluator.model is t.ema_model
    assert [h[0] for h in t.eval_history] == [3, 6]
    ds = t.evaluator.ds
    twin = DeviceEvaluator(t.ema_model, ds, 64, "cpu").run()
    live = DeviceEvaluator(t.model, ds, 64, "cpu").run()
    assert t.test_acc == twin.precision == hist[-1][2]
    assert t.eval_history[-1][2] == twin.loss
    # the two sets of weights really give different answers
    assert not torch.equal(t.flat_ema, t.fp.flat_master)
    lt, y = held_out_logits(t.ema_model, ds)
    ll, _ = held_out_logits(t.model, ds)
    differ = int((lt.argmax(1) != ll.argmax(1)).sum())
    assert differ >= 1
    assert not torch.equal(twin.confusion, live.confusion)
    assert twin.loss != live.loss
    # exact counts of the twin's own forward
    assert round(twin.precision * 150) == int((lt.argmax(1) == y).sum())
    saved = np.load(tmp_path / "td" / "worker0_time_acc.npy")
    assert saved[-1, 2] == twin.precision


# -- evaluator CLI --------------------------------------------------------------------

LINE = re.compile(r"Num examples: ([0-9]*)  Precision @ 1: ([\.0-9]*) "
                  r"Loss: ([\.0-9]*) Time: ([\.0-9]*)")


def run_eval_cli(tmp_path, tag, *extra, check=True):
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "src", "mnist_eval.py"),
         "--checkpoint_dir", str(tmp_path / "td"),
         "--eval_dir", str(tmp_path / tag),
         "--data_dir", str(tmp_path / "data"),
         "--run_once", "--model", "mlp", "--device", "cpu", *extra],
        capture_output=True, text=True, timeout=120)
    if not check:
        return out
    assert out.returncode == 0, out.stderr
    m = LINE.search(out.stdout)
    assert m, out.stdout
    return int(m.group(1)), float(m.group(2)), float(m.group(3))


def reference_eval(flat, tmp_path):
    """do_eval on a model loaded from `flat`, on the validation set the CLI
    reads."""
    from distributedmnist_amd.data import load_mnist
    from distributedmnist_amd.engine.evaluate import do_eval
    from distributedmnist_amd.models import build_model
    from distributedmnist_amd.parallel import FlatParams
    model = build_model("mlp", seed=66478, compute_dtype=torch.float32)
    FlatParams(model, device="cpu",
               compute_dtype=torch.float32).load_flat(flat)
    val = load_mnist(str(tmp_path / "data"), shard=False).validation
    return do_eval(model, torch.as_tensor(val.images),
                   torch.as_tensor(val.labels), torch.device("cpu"),
                   torch.float32)


def test_eval_cli_use_moving_average(tmp_path):
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    make_data(tmp_path)
    flags = train_flags(tmp_path, "td", "--moving_average_decay", "0.9",
                        "--initial_learning_rate", "0.5", "--max_steps", "6")
    t = Trainer(flags)
    t.train(make_dataset(flags, 0, 1, t.device, t.compute_dtype))
    acc_e, loss_e = reference_eval(t.flat_ema, tmp_path)
    acc_w, loss_w = reference_eval(t.fp.flat_master, tmp_path)
    assert loss_e != loss_w  # the comparison below can tell them apart
    for tag, extra in (("host", ()), ("dev", ("--device_data",
                                              "--eval_batch_size", "64"))):
        n, p, l = run_eval_cli(tmp_path, "ema_" + tag,
                               "--use_moving_average", *extra)
        assert n == 150 and p == float("%f" % acc_e)
        assert abs(l - loss_e) <= 1e-5 * loss_e + 1e-6  # %f: 6 decimals
        # without the flag: the raw weights, as before
        n, p, l = run_eval_cli(tmp_path, "raw_" + tag, *extra)
        assert n == 150 and p == float("%f" % acc_w)
        assert abs(l - loss_w) <= 1e-5 * loss_w + 1e-6
        assert abs(l - loss_e) > 1e-5 * loss_e + 1e-6


@pytest.mark.parametrize("extra", [(), ("--device_data",)],
                         ids=["host", "device_data"])
def test_eval_cli_errors_without_an_average(tmp_path, extra):
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    make_data(tmp_path)
    flags = train_flags(tmp_path, "td", "--max_steps", "2")
    t = Trainer(flags)
    t.train(make_dataset(flags, 0, 1, t.device, t.compute_dtype))
    out = run_eval_cli(tmp_path, "e", "--use_moving_average", *extra,
                       check=False)
    assert out.returncode != 0
    assert "--moving_average_decay" in out.stderr
    assert not LINE.search(out.stdout)  # no result line from the raw weights


# -- two gloo ranks ---------------------------------------------------------------------

def _rank_train(rank, world, port, train_dir, extra, q):
    import torch.distributed as dist
    init_pg(rank, world, port)
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    flags = build_train_parser().parse_args(
        ["--synthetic_data", "--train_dir", train_dir,
         "--batch_size", "16", "--max_steps", "6", "--model", "mlp",
         "--device", "cpu", "--save_interval_secs", "100000",
         "--moving_average_decay", "0.5"] + list(extra))
    t = Trainer(flags, rank=rank, world=world, local_rank=rank)
    t.train(make_dataset(flags, rank, world, t.device, t.compute_dtype))
    q.put((rank, t.flat_ema.numpy().tobytes(),
           t.fp.flat_master.numpy().tobytes()))
    dist.destroy_process_group()


@pytest.mark.timeout(240)
@pytest.mark.parametrize("extra", [
    (), ("--num_replicas_to_aggregate", "1"),
    ("--interval_method", "--interval_ms", "0")],
    ids=["full_sync", "k_of_n", "interval"])
def test_world2_average_identical_on_both_ranks(tmp_path, extra):
    out = spawn_collect(_rank_train, 2, args=(str(tmp_path / "td"), extra))
    (e0, w0), (e1, w1) = out[0], out[1]
    assert w0 == w1
    assert e0 == e1
    assert e0 != w0


# -- argument validation -------------------------------------------------------------------

def test_flag_default_and_range(tmp_path, capsys):
    from distributedmnist_amd.utils.flags import (build_eval_parser,
                                                  build_train_parser)
    p = build_train_parser()
    assert p.parse_args([]).moving_average_decay == 0.0
    assert p.parse_args(["--moving_average_decay", "0.999"]
                        ).moving_average_decay == 0.999
    for bad in ("1", "1.0", "-0.1", "2", "nan", "x"):
        with pytest.raises(SystemExit) as ei:
            p.parse_args(["--moving_average_decay", bad])
        assert ei.value.code == 2
    assert "--moving_average_decay" in capsys.readouterr().err
    e = build_eval_parser()
    assert e.parse_args([]).use_moving_average is False
    assert e.parse_args(["--use_moving_average"]).use_moving_average is True


def test_trainer_refuses_a_bad_decay(tmp_path):
    from distributedmnist_amd.engine.train import Trainer
    flags = train_flags(tmp_path, "td")
    for bad in (1.0, -0.5):
        flags.moving_average_decay = bad
        with pytest.raises(ValueError, match="moving_average_decay"):
            Trainer(flags)


def test_flag_off_builds_nothing(tmp_path):
    from distributedmnist_amd.engine.train import Trainer
    t = Trainer(train_flags(tmp_path, "td"))
    assert t.flat_ema is None and t.ema_model is None and t.ema_fp is None
    assert t.eval_model is t.model
