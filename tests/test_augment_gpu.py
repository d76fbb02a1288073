"""On-device affine augmentation on the GPU: batch_gather_aug_kernel against
the CPU reference (bit-exact on the bf16 bit patterns), the augmented gather
captured inside the hipGraph (full and two-graph split scope), graph against
eager, and evaluation untouched by the augment flags."""

import numpy as np
import pytest
import torch

from distributedmnist_amd.data import DeviceDataSet
from distributedmnist_amd.data.mnist_data import write_random_idx
from distributedmnist_amd.ops.cpu_ref import augment_table

pytestmark = pytest.mark.gpu

SEED = 66478
ONE = 65536
N_TRAIN, BATCH = 256, 64
SPE = N_TRAIN // BATCH
AUG = ("--augment_shift", "2", "--augment_rotate", "10",
       "--augment_scale", "0.1")

# integer shifts (all four borders, fully outside at +-28, one surviving
# corner), the identity, and one zoom-out entry at the builder's |a| bound
HAND = np.array(
    [(ONE, 0, 0, ONE, dx * ONE, dy * ONE)
     for dx, dy in ((3, -2), (-6, 6), (28, 0), (0, -28), (27, 27), (0, 0))]
    + [(4 * ONE, 0, 0, 4 * ONE, 0, 0)], dtype=np.int32)


def tables():
    return {
        "T1": augment_table(1, SEED, 8, 30, 0.4),
        "T7": augment_table(7, SEED, 8, 30, 0.4),
        "T4096": augment_table(4096, SEED, 8, 30, 0.4),
        "hand": HAND,
    }


def bits(x):
    return x.view(torch.int16).cpu()


def raw_set(n):
    rng = np.random.RandomState(n)
    img = rng.randint(0, 256, size=(n, 784), dtype=np.uint8)
    img[0, :256] = np.arange(256)  # every LUT entry
    img[n // 2] = (img[n // 2] > 127) * 255  # one 0/255 binary image
    lab = rng.randint(0, 10, size=n, dtype=np.uint8)
    return img, lab


def make_pair(n, table, seed=SEED):
    """The same uint8 set and table as a CPU (reference) and a GPU (kernel)
    data set, both bf16."""
    img, lab = raw_set(n)
    ref = DeviceDataSet(img, lab, seed=seed, dtype=torch.bfloat16,
                        aug_table=table)
    dev = DeviceDataSet(img, lab, seed=seed, dtype=torch.bfloat16,
                        device="cuda", aug_table=table)
    return ref, dev


# (1,1) single image; (37,5) partial last block; (65,64) longest cycle walk
# (128 codes for 65 values); (1000,1000) B == N
@pytest.mark.parametrize("n,b", [(1, 1), (37, 5), (65, 64), (1000, 1000)])
@pytest.mark.parametrize("name", ["T1", "T7", "T4096", "hand"])
def test_kernel_matches_cpu_reference_bit_exact(n, b, name):
    ref, dev = make_pair(n, tables()[name])
    assert dev.aug_table.is_cuda and dev.aug_table.dtype == torch.int32
    spe = n // b
    differs = False
    for step in (0, spe - 1, spe, 2 * spe + 1, 10 ** 9):
        ex, ey = ref.batch_at(step, b)
        x, y = dev.batch_at(step, b)
        assert x.is_cuda and x.dtype == torch.bfloat16
        assert x.shape == (b, 28, 28, 1) and y.dtype == torch.int64
        assert torch.equal(bits(x), bits(ex)), (n, b, name, step)
        assert torch.equal(y.cpu(), ey), (n, b, name, step)
        rx, ry = dev.batch_at(step, b, augment=False)
        assert torch.equal(ry, y)
        differs |= not torch.equal(bits(rx), bits(x))
    assert differs  # the augmented kernel ran, not the plain one


def test_kernel_leaves_neighbours_and_the_resident_set_alone():
    """Canary rows before and after the b written rows keep their fill;
    images and labels are read-only."""
    _, dev = make_pair(37, tables()["T7"])
    img0, lab0 = dev.images.clone(), dev.labels.clone()
    xb = torch.full((11, 28, 28, 1), 7.0, dtype=torch.bfloat16,
                    device="cuda")
    yb = torch.full((11,), -3, dtype=torch.int64, device="cuda")
    dev.gather_into(xb[3:8], yb[3:8], step=9)
    ex, ey = dev.batch_at(9, 5)
    assert torch.equal(bits(xb[3:8]), bits(ex)) and torch.equal(yb[3:8], ey)
    assert bool((xb[:3] == 7.0).all()) and bool((xb[8:] == 7.0).all())
    assert bool((yb[:3] == -3).all()) and bool((yb[8:] == -3).all())
    assert torch.equal(dev.images, img0) and torch.equal(dev.labels, lab0)


def test_step_dev_form_equals_host_step_form():
    ref, dev = make_pair(1000, tables()["T4096"])
    for step in (0, 9, 10, 21, 10 ** 9, 10 ** 12):
        sd = torch.tensor([step], dtype=torch.int64, device="cuda")
        x = torch.empty((96, 28, 28, 1), dtype=torch.bfloat16, device="cuda")
        y = torch.empty(96, dtype=torch.int64, device="cuda")
        dev.gather_into(x, y, step_dev=sd)
        ex, ey = dev.batch_at(step, 96)
        assert torch.equal(bits(x), bits(ex)) and torch.equal(y, ey), step
    rx, ry = ref.batch_at(10 ** 12, 96)  # the high step word, against CPU
    assert torch.equal(bits(x), bits(rx)) and torch.equal(y.cpu(), ry)


def test_binding_checks_the_table():
    from distributedmnist_amd import _C
    _, dev = make_pair(37, tables()["T7"])
    x = torch.empty((5, 28, 28, 1), dtype=torch.bfloat16, device="cuda")
    y = torch.empty(5, dtype=torch.int64, device="cuda")
    good = dev.aug_table
    for bad in (good.long(), good[:, :5].contiguous(), good[:0],
                good.t(), good.cpu(), good.reshape(-1)):
        with pytest.raises(RuntimeError):
            _C.ext().batch_gather_aug(dev.images, dev.labels, dev._lut, bad,
                                      x, y, SEED, 0)
    with pytest.raises(RuntimeError):  # batch_gather's own checks still hold
        _C.ext().batch_gather_aug(dev.images, dev.labels, dev._lut, good,
                                  x, y, SEED, -1)


# -- trainer integration ---------------------------------------------------------

@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("idx")
    write_random_idx(str(d), N_TRAIN, 16, seed=5)
    return str(d)


def make_trainer(data_dir, train_dir, *extra):
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    flags = build_train_parser().parse_args(
        ["--data_dir", data_dir, "--train_dir", str(train_dir),
         "--model", "lenet", "--batch_size", str(BATCH),
         "--save_interval_secs", "100000", *extra])
    t = Trainer(flags, device=torch.device("cuda:0"))
    ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
    return t, ds


def run_resident(data_dir, train_dir, steps, *extra):
    t, ds = make_trainer(data_dir, train_dir, "--device_data", *AUG, *extra)
    t.attach_dataset(ds)
    loss = None
    for _ in range(steps):
        _, loss, _, _ = t.resident_step()
    return float(loss), t


def test_augmented_gather_runs_inside_the_graph(data_dir, tmp_path):
    """9 replays across two epoch boundaries: the static slots hold exactly
    the augmented batch_at(step)."""
    t, ds = make_trainer(data_dir, tmp_path, "--device_data", *AUG)
    assert isinstance(ds, DeviceDataSet) and ds.aug_table is not None
    assert ds.aug_table.shape == (4096, 6)
    t.attach_dataset(ds)
    for step in range(9):
        assert t.step == step
        t.resident_step()
        g = t._graph
        assert g is not None and g.ds is ds, "capture must engage"
        ex, ey = ds.batch_at(step, BATCH)
        assert torch.equal(bits(g.static_x), bits(ex)), step
        assert torch.equal(g.static_y, ey), step
        rx, _ = ds.batch_at(step, BATCH, augment=False)
        assert not torch.equal(bits(g.static_x), bits(rx)), step
    assert int(g.step_dev.item()) == 9


def test_two_graph_split_capture_holds_the_augmented_gather(data_dir,
                                                            tmp_path):
    from distributedmnist_amd.engine.graphstep import GraphedStep
    t, ds = make_trainer(data_dir, tmp_path / "s", "--device_data", *AUG)
    t.attach_dataset(ds)
    g = GraphedStep(t, (BATCH, 28, 28, 1), split=True, dataset=ds)
    assert g.two_graph and g.ds is ds
    t._graph, t._graph_tried = g, True
    for step in range(9):
        t.resident_step()
        ex, ey = ds.batch_at(step, BATCH)
        assert torch.equal(bits(g.static_x), bits(ex)), step
        assert torch.equal(g.static_y, ey), step
    assert t.step == 9 and int(g.step_dev.item()) == 9


def test_graph_resident_matches_eager_resident(data_dir, tmp_path):
    """Bit-identical inputs; only the fp32-atomic order differs.  Bound: the
    project's own 5% (test_device_data_gpu.py)."""
    loss_g, tg = run_resident(data_dir, tmp_path / "g", 9)
    assert tg._graph is not None
    loss_e, te = run_resident(data_dir, tmp_path / "e", 9,
                              "--hip_graph", "off")
    assert te._graph is None
    print(f"augmented graph-resident loss {loss_g:.6f} eager-resident "
          f"{loss_e:.6f} delta {abs(loss_g - loss_e):.3e}")
    assert abs(loss_g - loss_e) < 0.05 * max(1.0, abs(loss_e)), \
        (loss_g, loss_e)


def test_evaluation_is_unchanged_by_the_augment_flags(data_dir, tmp_path):
    """Same seed -> identical initial weights; the evaluator reads the
    held-out set through range_into, which never augments: same loss bits,
    same counts.  Also over an evaluation set that itself carries a table."""
    from distributedmnist_amd.engine.device_eval import DeviceEvaluator
    from distributedmnist_amd.engine.train import make_eval_dataset
    out = []
    for tag, extra in (("p", ()), ("a", AUG)):
        t, _ = make_trainer(data_dir, tmp_path / tag, "--device_data",
                            "--eval_every_steps", "5", *extra)
        ev = t.attach_eval_dataset(make_eval_dataset(
            t.flags, 0, 1, t.device, t.compute_dtype))
        res = ev.run()
        out.append((res[:3], ev.loss_sum.clone(), ev.counts.clone()))
    t_img, t_lab = raw_set(150)
    for table in (None, tables()["T7"]):
        ds = DeviceDataSet(t_img, t_lab, seed=SEED, dtype=torch.bfloat16,
                           device="cuda", aug_table=table)
        ev = DeviceEvaluator(t.model, ds, 64, "cuda")
        res = ev.run()
        out.append((res[:3], ev.loss_sum.clone(), ev.counts.clone()))
    for a, b in ((out[0], out[1]), (out[2], out[3])):
        assert a[0] == b[0]
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        assert torch.equal(a[2], b[2]) and int(a[2][0]) > 0
