"""batch_gather_elastic_kernel on the GPU: bit-exact against the CPU
definition and, at alpha_q = 0, its affine sibling; the device-step form, what
it leaves alone, and the trainer with the gather captured in the hipGraph."""

import numpy as np
import pytest
import torch

from distributedmnist_amd.data import DeviceDataSet
from distributedmnist_amd.data.mnist_data import write_random_idx
from distributedmnist_amd.ops.cpu_ref import augment_table

pytestmark = pytest.mark.gpu

SEED = 66478
N_TRAIN, BATCH = 256, 64
ELASTIC = ("--device_data", "--augment_elastic", "34")


def bits(x):
    return x.view(torch.int16).cpu()


def empty(b):
    return (torch.empty((b, 28, 28, 1), dtype=torch.bfloat16, device="cuda"),
            torch.empty(b, dtype=torch.int64, device="cuda"))


def make_pair(n, alpha, sigma, table=None):
    """The same set as a CPU (reference) and a GPU (kernel) data set."""
    rng = np.random.RandomState(n)
    img = rng.randint(0, 256, size=(n, 784), dtype=np.uint8)
    img[0, :256] = np.arange(256)  # every LUT entry
    lab = rng.randint(0, 10, size=n, dtype=np.uint8)
    kw = dict(seed=SEED, dtype=torch.bfloat16, aug_table=table,
              augment_elastic=alpha, augment_elastic_sigma=sigma)
    return DeviceDataSet(img, lab, **kw), \
        DeviceDataSet(img, lab, device="cuda", **kw)


# (1,1) and (37,5) leave a half-empty last block; (65,64) longest cycle walk;
# (1000,1000) B == N
@pytest.mark.parametrize("n,b", [(1, 1), (37, 5), (65, 64), (1000, 1000)])
@pytest.mark.parametrize("alpha,sigma", [(34, 4), (8, 1), (64, 16)])
@pytest.mark.parametrize("affine", [False, True])
def test_kernel_matches_cpu_reference_bit_exact(n, b, alpha, sigma, affine):
    table = augment_table(7, SEED, 8, 30, 0.4) if affine else None
    ref, dev = make_pair(n, alpha, sigma, table)
    spe = n // b
    for step in (spe - 1, 2 * spe + 1):  # epoch 0 and a shuffled epoch
        ex, ey = ref.batch_at(step, b)
        x, y = dev.batch_at(step, b)
        assert torch.equal(bits(x), bits(ex)), (n, b, alpha, sigma, step)
        assert torch.equal(y.cpu(), ey)
        rx, _ = dev.batch_at(step, b, augment=False)
        assert not torch.equal(bits(rx), bits(x))  # the field did something


def test_zero_alpha_equals_the_affine_kernel_bit_for_bit():
    from distributedmnist_amd import _C
    _, dev = make_pair(1000, 34, 4, augment_table(4096, SEED, 8, 30, 0.4))
    out = []
    for op in ("elastic", "aug"):
        x, y = empty(96)
        head = (dev.images, dev.labels, dev._lut, dev.aug_table)
        if op == "elastic":
            _C.ext().batch_gather_elastic(*head, dev.elastic[0], 0, x, y,
                                          SEED, 23)
        else:
            _C.ext().batch_gather_aug(*head, x, y, SEED, 23)
        out.append((bits(x), y.cpu()))
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])
    for taps, alpha_q in ((dev.elastic[0].long(), 0), (dev.elastic[0][:31], 0),
                          (dev.elastic[0].cpu(), 0), (dev.elastic[0], -1),
                          (dev.elastic[0], 16385)):
        with pytest.raises(RuntimeError):
            _C.ext().batch_gather_elastic(*head, taps, alpha_q, x, y, SEED, 0)


def test_step_dev_form_equals_host_step_form():
    _, dev = make_pair(1000, 34, 4, augment_table(7, SEED, 8, 30, 0.4))
    for step in (0, 21, 10 ** 12):
        sd = torch.tensor([step], dtype=torch.int64, device="cuda")
        x, y = empty(96)
        dev.gather_into(x, y, step_dev=sd)
        ex, ey = dev.batch_at(step, 96)
        assert torch.equal(bits(x), bits(ex)) and torch.equal(y, ey), step


def test_kernel_leaves_neighbours_and_the_resident_set_alone():
    ref, dev = make_pair(37, 34, 4)
    img0, lab0 = dev.images.clone(), dev.labels.clone()
    xb = torch.full((11, 28, 28, 1), 7.0).to("cuda", torch.bfloat16)
    yb = torch.full((11,), -3, dtype=torch.int64, device="cuda")
    dev.gather_into(xb[3:8], yb[3:8], step=9)
    ex, ey = ref.batch_at(9, 5)
    assert torch.equal(bits(xb[3:8]), bits(ex))
    assert torch.equal(yb[3:8].cpu(), ey)
    assert bool((xb[:3] == 7.0).all()) and bool((xb[8:] == 7.0).all())
    assert bool((yb[:3] == -3).all()) and bool((yb[8:] == -3).all())
    assert torch.equal(dev.images, img0) and torch.equal(dev.labels, lab0)


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
    return t, make_dataset(flags, 0, 1, t.device, t.compute_dtype)


def test_trainer_gathers_in_both_graph_scopes_and_matches_eager(data_dir,
                                                                tmp_path):
    """9 replays across two epoch boundaries hold exactly batch_at(step), in
    the full and the two-graph split capture; then graph against eager: same
    inputs, other fp32-atomic order, the project's 5% bound
    (test_device_data_gpu.py)."""
    from distributedmnist_amd.engine.graphstep import GraphedStep
    loss = {}
    for tag, extra in (("g", ()), ("s", ()), ("e", ("--hip_graph", "off"))):
        t, ds = make_trainer(data_dir, tmp_path / tag, *ELASTIC, *extra)
        t.attach_dataset(ds)
        if tag == "s":
            g = GraphedStep(t, (BATCH, 28, 28, 1), split=True, dataset=ds)
            assert g.two_graph
            t._graph, t._graph_tried = g, True
        for step in range(9):
            _, loss[tag], _, _ = t.resident_step()
            if tag == "e":
                continue
            g = t._graph
            assert g is not None and g.ds is ds, "capture must engage"
            ex, ey = ds.batch_at(step, BATCH)
            assert torch.equal(bits(g.static_x), bits(ex)), (tag, step)
            assert torch.equal(g.static_y, ey), (tag, step)
            rx, _ = ds.batch_at(step, BATCH, augment=False)
            assert not torch.equal(bits(g.static_x), bits(rx)), step
        assert (t._graph is None) == (tag == "e")
    le = float(loss["e"])
    for tag in "gs":
        print(f"elastic {tag} loss {float(loss[tag]):.6f} eager {le:.6f}")
        assert abs(float(loss[tag]) - le) < 0.05 * max(1.0, abs(le)), tag


def test_evaluation_is_unchanged_by_the_elastic_flag(data_dir, tmp_path):
    from distributedmnist_amd.engine.train import make_eval_dataset
    out = []
    for tag, extra in (("p", ("--device_data",)), ("a", ELASTIC)):
        t, _ = make_trainer(data_dir, tmp_path / tag,
                            "--eval_every_steps", "5", *extra)
        ev = t.attach_eval_dataset(make_eval_dataset(
            t.flags, 0, 1, t.device, t.compute_dtype))
        res = ev.run()
        out.append((res[:3], ev.loss_sum.clone(), ev.counts.clone()))
    a, b = out
    assert a[0] == b[0]
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert torch.equal(a[2], b[2]) and int(a[2][0]) > 0
