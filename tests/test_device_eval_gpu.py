"""Device-resident evaluation on the GPU: range_gather_kernel and
softmax_eval_kernel against the CPU references, DeviceEvaluator graphed vs
eager vs a reference built here, and the trainer's --eval_every_steps next
to the training graph."""

import numpy as np
import pytest
import torch

from distributedmnist_amd.data import DeviceDataSet
from distributedmnist_amd.data.device_data import normalisation_lut
from distributedmnist_amd.data.mnist_data import write_random_idx
from distributedmnist_amd.ops import cpu_ref
from distributedmnist_amd.ops import functional as Fx

pytestmark = pytest.mark.gpu

# loss_sum against fp64: the derivable part is the fp32 summation, about
# 2*B*2^-24 relative (7e-5 at B = 600); the fast exp/log intrinsics are
# bounded, not derived
LOSS_RTOL = 1e-3


def bits(x):
    return x.view(torch.int16).cpu()


def make_pair(n):
    """The same uint8 set as a CPU (reference) and a GPU (kernel) data set,
    both bf16."""
    rng = np.random.RandomState(n)
    img = rng.randint(0, 256, size=(n, 784), dtype=np.uint8)
    img[0, :256] = np.arange(256)  # every LUT entry
    lab = rng.randint(0, 10, size=n, dtype=np.uint8)
    ref = DeviceDataSet(img, lab, dtype=torch.bfloat16)
    dev = DeviceDataSet(img, lab, dtype=torch.bfloat16, device="cuda")
    return ref, dev, img, lab


# -- range_gather ------------------------------------------------------------------

# (1,1,0) single image; (65,16,60) 5 live rows, the set ends inside a block
# on an odd image; (37,5,35) live/padding split inside one block; (37,8,40)
# all padding; (5,8,0) B > N; (1000,1000,0) B == N; (7500,96,7488) many blocks
@pytest.mark.parametrize("n,b,start", [(1, 1, 0), (65, 16, 60), (37, 5, 35),
                                       (37, 8, 40), (5, 8, 0),
                                       (1000, 1000, 0), (7500, 96, 7488)])
def test_range_gather_matches_cpu_reference_bit_exact(n, b, start):
    ref, dev, _, _ = make_pair(n)
    ex = torch.full((b, 28, 28, 1), 7.0, dtype=torch.bfloat16)
    ey = torch.full((b,), -3, dtype=torch.int64)
    ref.range_into(ex, ey, start=start)
    # sentinel-filled buffer three rows longer than the chunk
    xb = torch.full((b + 3, 28, 28, 1), 7.0, dtype=torch.bfloat16,
                    device="cuda")
    yb = torch.full((b + 3,), -3, dtype=torch.int64, device="cuda")
    dev.range_into(xb[:b], yb[:b], start=start)
    assert torch.equal(bits(xb[:b]), bits(ex)), (n, b, start)
    assert torch.equal(yb[:b].cpu(), ey), (n, b, start)
    assert bool((xb[b:] == 7.0).all()) and bool((yb[b:] == -3).all())
    live = max(0, min(b, n - start))
    assert bool((yb[live:b] == -1).all())
    assert not bits(xb[live:b]).any()  # +0.0, bit for bit
    # the device-cursor form
    x2 = torch.full((b, 28, 28, 1), 7.0, dtype=torch.bfloat16, device="cuda")
    y2 = torch.full((b,), -3, dtype=torch.int64, device="cuda")
    sd = torch.tensor([start], dtype=torch.int64, device="cuda")
    dev.range_into(x2, y2, start_dev=sd)
    assert torch.equal(bits(x2), bits(ex)) and torch.equal(y2.cpu(), ey)
    assert int(sd) == start  # the gather does not move the cursor


def test_range_gather_row_equals_training_gather_row():
    """Same image, same bits as batch_gather_kernel (epoch 0 = identity)."""
    _, dev, _, _ = make_pair(65)
    x, y = dev.batch_at(0, 16)
    x2 = torch.empty_like(x)
    y2 = torch.empty_like(y)
    dev.range_into(x2, y2, start=0)
    assert torch.equal(bits(x), bits(x2)) and torch.equal(y, y2)
    with pytest.raises(ValueError):
        dev.range_into(x2, y2)


# -- softmax_eval ------------------------------------------------------------------

def eval_case(B, C, seed):
    """bf16 logits with exact ties; labels with -1, C and, from row 256 on,
    a whole dead block of 256 rows."""
    g = torch.Generator().manual_seed(seed)
    logits = (2.0 * torch.randn(B, C, generator=g)).to(torch.bfloat16)
    labels = torch.randint(0, C, (B,), generator=g)
    for r in range(0, B, 7):  # two equal maxima, label on either of them
        lo, hi = r % (C - 1), C - 1
        logits[r] = -1.0
        logits[r, lo] = logits[r, hi] = 2.5
        labels[r] = lo if (r // 7) % 2 == 0 else hi
    labels[1::13] = -1
    labels[2::17] = C
    labels[256:512] = -1
    return logits, labels


def fp64_loss(logits, labels):
    C = logits.shape[1]
    live = (labels >= 0) & (labels < C)
    lf = logits.double()[live]
    return float((torch.logsumexp(lf, dim=1)
                  - lf.gather(1, labels[live].view(-1, 1)).squeeze(1)).sum())


def state(C, device):
    return (torch.zeros(1, device=device),
            torch.zeros(2 + C * C, dtype=torch.int32, device=device))


def check_against_reference(B, C):
    logits, labels = eval_case(B, C, seed=B)
    loss_r, counts_r = state(C, "cpu")
    pred_r = torch.zeros(B, dtype=torch.uint8)
    cpu_ref.softmax_eval(logits, labels, loss_r, counts_r, pred=pred_r)
    loss_d, counts_d = state(C, "cuda")
    pred_d = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    cursor = torch.tensor([40], dtype=torch.int64, device="cuda")
    Fx.softmax_eval(logits.cuda(), labels.cuda(), loss_d, counts_d,
                    pred=pred_d, cursor_dev=cursor)
    assert torch.equal(counts_d.cpu(), counts_r), (B, C)
    assert torch.equal(pred_d.cpu(), pred_r), (B, C)
    assert int(cursor) == 40 + B
    conf = counts_d[2:].view(C, C)
    assert int(conf.sum()) == int(counts_d[0])
    assert int(conf.trace()) == int(counts_d[1])
    want = fp64_loss(logits, labels)
    if int(counts_r[0]) == 0:
        assert float(loss_d) == 0.0
        return
    rel = abs(float(loss_d) - want) / want
    print(f"softmax_eval B={B} C={C}: loss_sum {float(loss_d):.6f} fp64 "
          f"{want:.6f} rel err {rel:.3e}")
    assert rel <= LOSS_RTOL, (B, C, rel)


# 1 and 64: the single-block path; 257: a partial second block; 600: several
# blocks, one of them (rows 256..511) all dead
@pytest.mark.parametrize("B", [1, 64, 257, 600])
def test_softmax_eval_c10_matches_reference(B):
    check_against_reference(B, 10)


def test_softmax_eval_runtime_c_path():
    check_against_reference(300, 7)


def test_softmax_eval_accumulates_and_repeats_bitwise():
    C = 10
    logits, labels = eval_case(600, C, seed=5)
    lg, lb = logits.cuda(), labels.cuda()

    def sequence():
        loss, counts = state(C, "cuda")
        cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
        for s in (0, 257, 514):  # 257 + 257 + 86 rows
            e = min(s + 257, 600)
            Fx.softmax_eval(lg[s:e].contiguous(), lb[s:e].contiguous(), loss,
                            counts, cursor_dev=cursor)
        return loss, counts, cursor

    loss_a, counts_a, cursor = sequence()
    assert int(cursor) == 600
    loss_b, counts_b = state(C, "cuda")
    Fx.softmax_eval(lg, lb, loss_b, counts_b)
    assert torch.equal(counts_a, counts_b)
    want = fp64_loss(logits, labels)
    assert abs(float(loss_a) - want) / want <= LOSS_RTOL
    # the whole sequence again from reset: the same bits
    loss_c, counts_c, _ = sequence()
    assert torch.equal(counts_a, counts_c)
    assert torch.equal(loss_a.view(torch.int32), loss_c.view(torch.int32))


# -- DeviceEvaluator -------------------------------------------------------------------

N, B = 150, 64


def lenet(seed=66478):
    from distributedmnist_amd.models import build_model
    from distributedmnist_amd.parallel import FlatParams
    model = build_model("lenet", seed=seed,
                        compute_dtype=torch.bfloat16).to("cuda")
    fp = FlatParams(model, device=torch.device("cuda"),
                    compute_dtype=torch.bfloat16)
    return model, fp


def evaluator(model, ds, b=B):
    from distributedmnist_amd.engine.device_eval import DeviceEvaluator
    return DeviceEvaluator(model, ds, b, "cuda")


def test_evaluator_graph_equals_eager_and_reference(monkeypatch):
    ref, dev, _, _ = make_pair(N)
    model, _ = lenet()
    ev = evaluator(model, dev)
    assert ev.graph is not None, "capture must engage"
    res = ev.run()
    counts_g = ev.counts.clone()
    loss_g = ev.loss_sum.clone()
    monkeypatch.setenv("DMNIST_EVAL_GRAPH", "0")
    ev_e = evaluator(model, dev)
    assert ev_e.graph is None
    res_e = ev_e.run()
    assert torch.equal(ev_e.counts, counts_g)
    assert torch.equal(ev_e.loss_sum.view(torch.int32),
                       loss_g.view(torch.int32))
    assert res_e[:3] == res[:3]
    # reference: the same padded chunks from the CPU set, forward on the
    # GPU, statistics by the CPU reference
    loss_r, counts_r = state(10, "cpu")
    loss64 = 0.0
    for start in range(0, N, B):
        x = torch.empty((B, 28, 28, 1), dtype=torch.bfloat16)
        y = torch.empty(B, dtype=torch.int64)
        ref.range_into(x, y, start=start)
        with torch.no_grad():
            logits = model(x.cuda(), train=False).cpu()
        cpu_ref.softmax_eval(logits, y, loss_r, counts_r)
        loss64 += fp64_loss(logits, y)
    assert torch.equal(counts_g.cpu(), counts_r)
    rel = abs(float(loss_g) - loss64) / loss64
    print(f"evaluator loss_sum {float(loss_g):.6f} fp64 {loss64:.6f} "
          f"rel err {rel:.3e}")
    assert rel <= LOSS_RTOL
    assert res.num_examples == N and int(res.confusion.sum()) == N
    assert res.precision == int(counts_r[1]) / N
    # a second run: the reset works under replay too
    again = ev.run()
    assert again[:3] == res[:3] and torch.equal(again.confusion, res.confusion)


def test_evaluator_agrees_with_do_eval():
    from distributedmnist_amd.engine.evaluate import do_eval
    n = 128
    _, dev, img, lab = make_pair(n)
    model, _ = lenet()
    res = evaluator(model, dev).run()
    images = normalisation_lut()[torch.from_numpy(img).long()].view(
        n, 28, 28, 1)
    acc, loss = do_eval(model, images, torch.from_numpy(lab).long(),
                        torch.device("cuda"), torch.bfloat16, batch_size=64)
    assert round(res.precision * n) == round(acc * n)
    assert abs(res.precision * n - round(res.precision * n)) < 1e-6
    print(f"DeviceEvaluator loss {res.loss:.6f} do_eval loss {loss:.6f}")


def test_evaluator_follows_in_place_weight_updates():
    _, dev, _, _ = make_pair(N)
    model, fp = lenet()
    ev = evaluator(model, dev)
    graph = ev.graph
    assert graph is not None
    before = ev.run()
    g = torch.Generator().manual_seed(1)
    fp.load_flat(fp.flat_master.cpu()
                 + 0.05 * torch.randn(fp.total, generator=g))
    after = ev.run()
    assert ev.graph is graph  # no re-capture
    fresh = evaluator(model, dev).run()
    assert after[:3] == fresh[:3]
    assert torch.equal(after.confusion, fresh.confusion)
    assert after.loss != before.loss


# -- trainer -----------------------------------------------------------------------------

def run_training(data_dir, train_dir, *extra):
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    flags = build_train_parser().parse_args(
        ["--data_dir", data_dir, "--train_dir", str(train_dir),
         "--model", "lenet", "--batch_size", "64", "--max_steps", "7",
         "--save_interval_secs", "100000", "--device_data", *extra])
    t = Trainer(flags, device=torch.device("cuda:0"))
    hist = t.train(make_dataset(flags, 0, 1, t.device, t.compute_dtype))
    return t, hist


def test_trainer_eval_graph_next_to_training_graph(tmp_path):
    data_dir = str(tmp_path / "data")
    write_random_idx(data_dir, 256, 150, seed=5)
    t, hist = run_training(data_dir, tmp_path / "on",
                           "--eval_every_steps", "3")
    assert t._graph is not None and t.evaluator.graph is not None
    assert t.evaluator.ds.num_examples == 150
    assert [h[0] for h in t.eval_history] == [3, 6, 7]
    p3, p6, p7 = (h[1] for h in t.eval_history)
    assert [h[2] for h in hist] == [0.0, 0.0, p3, p3, p3, p6, p7]
    t0, hist0 = run_training(data_dir, tmp_path / "off")
    assert t0.evaluator is None and [h[2] for h in hist0] == [0.0] * 7
    # evaluation must not disturb the training state: the project's
    # graph/eager bound on every step loss
    for step, (a, b) in enumerate(zip(hist, hist0)):
        print(f"step {step + 1}: loss with eval {a[3]:.6f} without "
              f"{b[3]:.6f}")
        assert abs(a[3] - b[3]) < 0.05 * max(1.0, abs(b[3])), (step, a, b)
    fresh = evaluator(t.model, t.evaluator.ds, t.evaluator.B).run()
    assert fresh.num_examples == 150 and fresh.precision == p7
