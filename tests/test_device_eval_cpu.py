"""Device-resident evaluation, CPU side: the range_gather / softmax_eval
references, DeviceEvaluator through the reference ops, the trainer's
--eval_every_steps, the sharded two-rank evaluation and the evaluator CLI's
--device_data path."""

import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from mp_utils import init_pg, spawn_collect

from distributedmnist_amd.data import DeviceDataSet
from distributedmnist_amd.data.device_data import normalisation_lut
from distributedmnist_amd.data.mnist_data import write_random_idx
from distributedmnist_amd.ops import cpu_ref
from distributedmnist_amd.ops import functional as Fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def raw_set(n, seed=3):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, size=(n, 784), dtype=np.uint8)
    img[0, :256] = np.arange(256)  # every LUT entry is exercised
    lab = rng.randint(0, 10, size=n, dtype=np.uint8)
    return img, lab


# -- cpu_ref.range_gather -----------------------------------------------------

@pytest.mark.parametrize("start", [0, 48, 60, 64, 65, 1000])
def test_range_gather_reference(start):
    N, B = 65, 16
    img, lab = raw_set(N)
    lut = normalisation_lut()
    x = torch.full((B, 28, 28, 1), 7.0)
    y = torch.full((B,), -3, dtype=torch.int64)
    cpu_ref.range_gather(torch.from_numpy(img), torch.from_numpy(lab), lut,
                         x, y, start)
    live = max(0, min(B, N - start))
    ex = lut.numpy()[img[start:start + live]].reshape(live, 28, 28, 1)
    assert np.array_equal(x[:live].numpy(), ex)
    assert np.array_equal(y[:live].numpy(),
                          lab[start:start + live].astype(np.int64))
    # padding rows: exactly +0.0 (not merely == 0), label -1
    pad = x[live:].numpy().view(np.uint32)
    assert not pad.any()
    assert bool((y[live:] == -1).all())


def test_range_into_wants_exactly_one_start():
    img, lab = raw_set(65)
    ds = DeviceDataSet(img, lab)
    x = torch.empty((16, 28, 28, 1))
    y = torch.empty(16, dtype=torch.int64)
    with pytest.raises(ValueError):
        ds.range_into(x, y)
    with pytest.raises(ValueError):
        ds.range_into(x, y, start=0, start_dev=torch.zeros(1, dtype=torch.int64))
    # the device form reads the same chunk as the host form
    ds.range_into(x, y, start_dev=torch.tensor([60]))
    ex = torch.empty_like(x)
    ey = torch.empty_like(y)
    ds.range_into(ex, ey, start=60)
    assert torch.equal(x, ex) and torch.equal(y, ey)
    assert y[5:].tolist() == [-1] * 11


def test_random_and_test_split(tmp_path):
    a = DeviceDataSet.random(100, 4242)
    b = DeviceDataSet.random(100, 4242)
    assert a.num_examples == 100 and a.images.dtype == torch.uint8
    assert torch.equal(a.images, b.images) and torch.equal(a.labels, b.labels)
    assert int(a.labels.max()) < 10
    shard = DeviceDataSet.random(100, 4242, worker_id=1, n_workers=3)
    assert torch.equal(shard.images, a.images[1::3])
    from distributedmnist_amd.data import load_device_mnist
    from distributedmnist_amd.data.mnist_data import (extract_images_u8,
                                                      extract_labels)
    write_random_idx(str(tmp_path), 32, 21, seed=1)
    img = extract_images_u8(str(tmp_path / "t10k-images-idx3-ubyte.gz"))
    lab = extract_labels(str(tmp_path / "t10k-labels-idx1-ubyte.gz"))
    ds = load_device_mnist(str(tmp_path), split="test")
    assert ds.num_examples == 21 and np.array_equal(ds.images.numpy(), img)
    ds = load_device_mnist(str(tmp_path), split="test", worker_id=1,
                           n_workers=2, subset=4)
    assert np.array_equal(ds.images.numpy(), img[1::2][:4])
    assert np.array_equal(ds.labels.numpy(), lab[1::2][:4].astype(np.uint8))
    assert load_device_mnist(str(tmp_path)).num_examples == 32  # default
    with pytest.raises(ValueError):
        load_device_mnist(str(tmp_path), split="validation")


# -- cpu_ref.softmax_eval ---------------------------------------------------------

def loop_reference(logits, labels):
    """Plain fp64 loop: (loss_sum, live, correct, confusion, pred)."""
    B, C = logits.shape
    loss, live, correct = 0.0, 0, 0
    conf = [[0] * C for _ in range(C)]
    pred = []
    for b in range(B):
        row = [float(v) for v in logits[b]]
        t = int(labels[b])
        if not 0 <= t < C:
            pred.append(255)
            continue
        m = max(row)
        p = min(c for c in range(C) if row[c] == m)  # lowest maximal index
        lse = m + math.log(sum(math.exp(v - m) for v in row))
        loss += lse - row[t]
        live += 1
        correct += int(p == t)
        conf[t][p] += 1
        pred.append(p)
    return loss, live, correct, conf, pred


def eval_case(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, C, generator=g)
    labels = torch.randint(0, C, (B,), generator=g)
    return logits, labels


def fresh_state(C):
    return torch.zeros(1), torch.zeros(2 + C * C, dtype=torch.int32)


def test_softmax_eval_reference_against_fp64_loop():
    C = 10
    logits, labels = eval_case(40, C, 0)
    labels[3] = -1
    labels[4] = C       # one past the last class: not live
    labels[5] = 255
    # exact ties, lower index must win in both directions
    logits[6] = 0.0
    logits[6, 2] = logits[6, 7] = 3.0
    labels[6] = 2       # lower index is the label: correct
    logits[7] = 0.0
    logits[7, 2] = logits[7, 7] = 3.0
    labels[7] = 7       # higher index is the label: wrong
    loss_sum, counts = fresh_state(C)
    pred = torch.zeros(40, dtype=torch.uint8)
    cpu_ref.softmax_eval(logits, labels, loss_sum, counts, pred=pred)
    loss, live, correct, conf, epred = loop_reference(logits, labels)
    assert live == 37 and counts[0] == live and counts[1] == correct
    assert counts[2:].view(C, C).tolist() == conf
    assert pred.tolist() == epred
    assert pred[6] == 2 and pred[7] == 2
    assert pred[3] == pred[4] == pred[5] == 255
    assert abs(float(loss_sum) - loss) <= 1e-5 * loss
    conf_t = counts[2:].view(C, C)
    assert int(conf_t.sum()) == int(counts[0])
    assert int(conf_t.trace()) == int(counts[1])


def test_softmax_eval_accumulates():
    C = 10
    logits, labels = eval_case(90, C, 1)
    labels[::11] = -1
    loss_a, counts_a = fresh_state(C)
    cursor = torch.zeros(1, dtype=torch.int64)
    for s in (0, 30, 60):
        Fx.softmax_eval(logits[s:s + 30], labels[s:s + 30], loss_a, counts_a,
                        cursor_dev=cursor)
    loss_b, counts_b = fresh_state(C)
    Fx.softmax_eval(logits, labels, loss_b, counts_b)
    assert int(cursor) == 90
    assert torch.equal(counts_a, counts_b)
    assert abs(float(loss_a) - float(loss_b)) <= 1e-5 * float(loss_b)


# -- DeviceEvaluator on CPU -----------------------------------------------------

N, B = 150, 64  # tail of 22 rows


def build(model_name, seed=66478):
    from distributedmnist_amd.models import build_model
    from distributedmnist_amd.parallel import FlatParams
    model = build_model(model_name, seed=seed, compute_dtype=torch.float32)
    fp = FlatParams(model, device="cpu", compute_dtype=torch.float32)
    return model, fp


def whole_set_reference(model, img, lab):
    """One forward over the whole set + the fp64 loop."""
    x = normalisation_lut()[torch.from_numpy(img).long()].view(-1, 28, 28, 1)
    with torch.no_grad():
        logits = model(x, train=False)
    return logits, loop_reference(logits, torch.from_numpy(lab).long())


@pytest.mark.parametrize("model_name", ["mlp", "lenet"])
def test_evaluator_matches_whole_set_forward(model_name):
    from distributedmnist_amd.engine.device_eval import DeviceEvaluator
    img, lab = raw_set(N, seed=11)
    model, _ = build(model_name)
    ev = DeviceEvaluator(model, DeviceDataSet(img, lab), B, "cpu")
    assert ev.graph is None and ev.n_chunks == 3
    res = ev.run()
    _, (loss, live, correct, conf, _) = whole_set_reference(model, img, lab)
    assert res.num_examples == N == live
    assert res.precision == correct / N
    assert abs(res.loss - loss / N) <= 1e-5 * (loss / N)
    assert res.confusion.dtype == torch.int64
    assert res.confusion.tolist() == conf
    assert int(res.confusion.sum()) == N
    # two consecutive runs: the reset works
    again = ev.run()
    assert again[:3] == res[:3] and torch.equal(again.confusion, res.confusion)
    # one extra chunk past the end is all padding and changes nothing
    ev.reset()
    for _ in range(ev.n_chunks + 1):
        ev.step_chunk()
    assert int(ev.cursor) == (ev.n_chunks + 1) * B
    extra = ev.result()
    assert extra[:3] == res[:3] and torch.equal(extra.confusion, res.confusion)


# -- trainer ---------------------------------------------------------------------

def train_flags(tmp_path, *extra):
    from distributedmnist_amd.utils.flags import build_train_parser
    return build_train_parser().parse_args(
        ["--data_dir", str(tmp_path / "data"),
         "--train_dir", str(tmp_path / "td"), "--device", "cpu",
         "--model", "mlp", "--batch_size", "64", "--max_steps", "7",
         "--save_interval_secs", "100000", *extra])


def test_trainer_evaluates_every_n_steps_and_at_the_end(tmp_path):
    from distributedmnist_amd.engine.device_eval import DeviceEvaluator
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    write_random_idx(str(tmp_path / "data"), 256, 150, seed=2)
    flags = train_flags(tmp_path, "--eval_every_steps", "3",
                        "--eval_batch_size", "64",
                        "--save_results_period", "1")
    t = Trainer(flags)
    assert t.evaluator is None  # built by train(), not before
    hist = t.train(make_dataset(flags, 0, 1, t.device, t.compute_dtype))
    assert isinstance(t.evaluator, DeviceEvaluator)
    assert t.evaluator.ds.num_examples == 150 and t.evaluator.B == 64
    assert [h[0] for h in t.eval_history] == [3, 6, 7]
    p3, p6, p7 = (h[1] for h in t.eval_history)
    assert [h[2] for h in hist] == [0.0, 0.0, p3, p3, p3, p6, p7]
    # the last entry is the evaluator's own result on the final weights
    final = t.evaluator.run()
    assert final.num_examples == 150 and final.precision == p7
    saved = np.load(tmp_path / "td" / "worker0_time_acc.npy")
    assert saved[:, 2].tolist() == [h[2] for h in hist]


def test_trainer_without_the_flag_builds_nothing(tmp_path):
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    write_random_idx(str(tmp_path / "data"), 256, 150, seed=2)
    flags = train_flags(tmp_path)
    assert flags.eval_every_steps == 0 and flags.eval_batch_size == 1000
    t = Trainer(flags)
    hist = t.train(make_dataset(flags, 0, 1, t.device, t.compute_dtype))
    assert t.evaluator is None and t.eval_history == []
    assert [h[2] for h in hist] == [0.0] * 7


def test_eval_every_steps_refuses_interval_method(tmp_path):
    from distributedmnist_amd.engine.train import Trainer
    flags = train_flags(tmp_path, "--eval_every_steps", "3",
                        "--interval_method")
    with pytest.raises(ValueError, match="interval_method"):
        Trainer(flags)


def test_trainer_synthetic_uses_the_seeded_stand_in(tmp_path):
    from distributedmnist_amd.engine.train import make_eval_dataset
    flags = train_flags(tmp_path, "--synthetic_data")
    ds = make_eval_dataset(flags, 1, 2, torch.device("cpu"), torch.float32)
    ref = DeviceDataSet.random(10000, 4242)
    assert ds.num_examples == 5000
    assert torch.equal(ds.images, ref.images[1::2])


# -- two gloo ranks ----------------------------------------------------------------

SHARD_SEED = 11


def _rank_eval(rank, world, port, q):
    import torch.distributed as dist
    from distributedmnist_amd.engine.device_eval import DeviceEvaluator
    init_pg(rank, world, port)
    img, lab = raw_set(N, seed=SHARD_SEED)
    model, _ = build("mlp")
    ds = DeviceDataSet(img, lab, worker_id=rank, n_workers=world)
    ev = DeviceEvaluator(model, ds, B, "cpu", rank=rank, world=world)
    calls = []
    orig = dist.all_reduce

    def counting(*a, **k):
        calls.append(1)
        return orig(*a, **k)

    dist.all_reduce = counting
    res = ev.run()
    dist.all_reduce = orig
    dist.barrier()
    dist.destroy_process_group()
    q.put((rank, res.num_examples, res.precision, res.loss,
           res.confusion.tolist(), len(calls)))


def test_sharded_evaluation_two_ranks():
    from distributedmnist_amd.engine.device_eval import DeviceEvaluator
    img, lab = raw_set(N, seed=SHARD_SEED)
    model, _ = build("mlp")
    one = DeviceEvaluator(model, DeviceDataSet(img, lab), B, "cpu").run()
    logits, _ = whole_set_reference(model, img, lab)
    top2 = logits.float().topk(2, dim=1).values
    near = int(((top2[:, 0] - top2[:, 1]) < 1e-3).sum())
    # an input where many rows sit on a near-tie would check nothing
    assert near <= N // 20, near
    out = spawn_collect(_rank_eval, 2)
    assert out[0] == out[1]  # every rank gets the full result
    n, precision, loss, conf, n_reduce = out[0]
    assert n_reduce == 1  # exactly one all_reduce per evaluation
    assert n == N and sum(map(sum, conf)) == N
    correct = round(precision * n)
    assert abs(correct - round(one.precision * N)) <= near
    assert abs(loss - one.loss) <= 1e-4 * one.loss


# -- evaluator CLI -------------------------------------------------------------------

LINE = re.compile(r"Num examples: ([0-9]*)  Precision @ 1: ([\.0-9]*) "
                  r"Loss: ([\.0-9]*) Time: ([\.0-9]*)")


def run_eval_cli(tmp_path, tag, *extra):
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "src", "mnist_eval.py"),
         "--checkpoint_dir", str(tmp_path / "td"),
         "--eval_dir", str(tmp_path / tag),
         "--data_dir", str(tmp_path / "data"),
         "--run_once", "--model", "mlp", "--device", "cpu", *extra],
        capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    m = LINE.search(out.stdout)
    assert m, out.stdout
    assert re.search(r"Succesfully loaded model from \S+ at step=3\.",
                     out.stdout), out.stdout
    return int(m.group(1)), float(m.group(2)), float(m.group(3)), out


def test_eval_cli_device_data_prints_the_same_result(tmp_path):
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    write_random_idx(str(tmp_path / "data"), 256, 150, seed=2)
    flags = train_flags(tmp_path, "--max_steps", "3")
    t = Trainer(flags)
    t.train(make_dataset(flags, 0, 1, t.device, t.compute_dtype))
    n0, p0, l0, _ = run_eval_cli(tmp_path, "eval_host")
    n1, p1, l1, out = run_eval_cli(tmp_path, "eval_dev", "--device_data",
                                   "--eval_batch_size", "64", "--confusion")
    assert n0 == n1 == 150
    assert p1 == p0
    assert abs(l1 - l0) <= 1e-5 * l0 + 1e-6  # %f prints 6 decimals
    conf = np.load(tmp_path / "eval_dev" / "confusion-3.npy")
    assert conf.shape == (10, 10) and conf.sum() == 150
    assert "recall" not in out.stdout  # the scrapers read stdout
