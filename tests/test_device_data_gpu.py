"""Device-resident input pipeline on the GPU: batch_gather_kernel against
the CPU reference (bit-exact), the gather captured inside the hipGraph, and
the resident trajectories against the eager and the host-fed ones."""

import numpy as np
import pytest
import torch

from distributedmnist_amd.data import DeviceDataSet
from distributedmnist_amd.data.mnist_data import write_random_idx

pytestmark = pytest.mark.gpu

SEED = 66478
N_TRAIN, BATCH = 256, 64
SPE = N_TRAIN // BATCH


def bits(x):
    return x.view(torch.int16).cpu()


def make_pair(n, seed=SEED):
    """The same uint8 set as a CPU (reference) and a GPU (kernel) data set,
    both bf16."""
    rng = np.random.RandomState(n)
    img = rng.randint(0, 256, size=(n, 784), dtype=np.uint8)
    img[0, :256] = np.arange(256)  # every LUT entry
    lab = rng.randint(0, 10, size=n, dtype=np.uint8)
    ref = DeviceDataSet(img, lab, seed=seed, dtype=torch.bfloat16)
    dev = DeviceDataSet(img, lab, seed=seed, dtype=torch.bfloat16,
                        device="cuda")
    return ref, dev


# (1,1) single image; (37,5) partial last block; (65,64) worst cycle-walk
# domain (128 codes for 65 values); (1000,1000) B == N; (7500,96) many blocks
@pytest.mark.parametrize("n,b", [(1, 1), (37, 5), (65, 64), (1000, 1000),
                                 (7500, 96)])
def test_kernel_matches_cpu_reference_bit_exact(n, b):
    ref, dev = make_pair(n)
    spe = n // b
    for step in (0, spe - 1, spe, 2 * spe + 1, 10 ** 9):
        ex, ey = ref.batch_at(step, b)
        x, y = dev.batch_at(step, b)
        assert x.is_cuda and x.dtype == torch.bfloat16
        assert x.shape == (b, 28, 28, 1) and y.dtype == torch.int64
        assert torch.equal(bits(x), bits(ex)), (n, b, step)
        assert torch.equal(y.cpu(), ey), (n, b, step)


def test_kernel_leaves_the_rest_of_the_buffer_alone():
    """Partial last block: nothing is written past image B-1."""
    _, dev = make_pair(37)
    xb = torch.full((8, 28, 28, 1), 7.0, dtype=torch.bfloat16, device="cuda")
    yb = torch.full((8,), -3, dtype=torch.int64, device="cuda")
    dev.gather_into(xb[:5], yb[:5], step=9)
    ex, ey = dev.batch_at(9, 5)
    assert torch.equal(bits(xb[:5]), bits(ex)) and torch.equal(yb[:5], ey)
    assert bool((xb[5:] == 7.0).all()) and bool((yb[5:] == -3).all())


def test_step_dev_form_equals_host_step_form():
    _, dev = make_pair(7500)
    for step in (0, 77, 78, 157, 10 ** 9, 10 ** 12):
        sd = torch.tensor([step], dtype=torch.int64, device="cuda")
        x = torch.empty((96, 28, 28, 1), dtype=torch.bfloat16, device="cuda")
        y = torch.empty(96, dtype=torch.int64, device="cuda")
        dev.gather_into(x, y, step_dev=sd)
        ex, ey = dev.batch_at(step, 96)
        assert torch.equal(bits(x), bits(ex)) and torch.equal(y, ey), step
    with pytest.raises(ValueError):
        dev.gather_into(x, y)  # neither step nor step_dev
    with pytest.raises(ValueError):
        dev.batch_at(0, 7501)


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
    t, ds = make_trainer(data_dir, train_dir, "--device_data", *extra)
    t.attach_dataset(ds)
    loss = None
    for _ in range(steps):
        _, loss, _, _ = t.resident_step()
    return float(loss), t


def test_gather_runs_inside_the_graph(data_dir, tmp_path, monkeypatch):
    """9 resident steps (two epoch boundaries): after every replay the
    graph's static slots hold exactly batch_at(step), and no copy_ ever
    targets them — the batch is built by the captured kernel."""
    t, ds = make_trainer(data_dir, tmp_path, "--device_data")
    assert isinstance(ds, DeviceDataSet) and t.compute_dtype == torch.bfloat16
    t.attach_dataset(ds)
    copied_into_slots = []
    orig = torch.Tensor.copy_

    def spy(self, *a, **k):
        g = t._graph
        if g is not None and self.data_ptr() in (g.static_x.data_ptr(),
                                                 g.static_y.data_ptr()):
            copied_into_slots.append(tuple(self.shape))
        return orig(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "copy_", spy)
    for step in range(9):
        assert t.step == step
        t.resident_step()
        g = t._graph
        assert g is not None and g.ds is ds, "capture must engage"
        ex, ey = ds.batch_at(step, BATCH)
        assert torch.equal(bits(g.static_x), bits(ex)), step
        assert torch.equal(g.static_y, ey), step
    assert int(g.step_dev.item()) == 9
    assert copied_into_slots == []
    with pytest.raises(RuntimeError):
        g.run(ex, ey)  # a resident graph would overwrite a passed-in batch


def test_graph_resident_matches_eager_resident(data_dir, tmp_path):
    """Bit-identical inputs; only the fp32-atomic order differs.  Bound:
    the project's own (test_two_graph_split_matches_eager_numerics)."""
    loss_g, tg = run_resident(data_dir, tmp_path / "g", 9)
    assert tg._graph is not None
    loss_e, te = run_resident(data_dir, tmp_path / "e", 9,
                              "--hip_graph", "off")
    assert te._graph is None
    print(f"graph-resident loss {loss_g:.6f} eager-resident {loss_e:.6f} "
          f"delta {abs(loss_g - loss_e):.3e}")
    assert abs(loss_g - loss_e) < 0.05 * max(1.0, abs(loss_e)), \
        (loss_g, loss_e)


def test_device_path_matches_host_path_first_epoch(data_dir, tmp_path):
    """Epoch 0 is unshuffled in both; the host path's fp32->bf16 cast
    rounds as the LUT does: bit-equal batches, losses within the 5% bound."""
    th, host = make_trainer(data_dir, tmp_path / "h")
    td, dev = make_trainer(data_dir, tmp_path / "d", "--device_data")
    td.attach_dataset(dev)
    loss_h = loss_d = None
    for step in range(SPE):
        x, y = th.to_device(*host.next_batch(BATCH))
        ex, ey = dev.batch_at(step, BATCH)
        assert torch.equal(bits(x), bits(ex)), step
        assert torch.equal(y, ey), step
        _, loss_h, _, _ = th.graph_or_eager_step(x, y)
        _, loss_d, _, _ = td.resident_step()
    loss_h, loss_d = float(loss_h), float(loss_d)
    print(f"host-fed loss {loss_h:.6f} device-data {loss_d:.6f} "
          f"delta {abs(loss_h - loss_d):.3e}")
    assert abs(loss_d - loss_h) < 0.05 * max(1.0, abs(loss_h)), \
        (loss_d, loss_h)


def test_two_graph_split_capture_holds_the_gather(data_dir, tmp_path):
    """The multi-rank capture scope (graph A = forward + fc backward, graph
    B = conv backward, eager tail), built here at world 1 so no process
    group is needed: the gather sits at the head of graph A, the slots hold
    batch_at(step) after every replay, and the trajectory tracks the eager
    resident one (same 5% bound)."""
    from distributedmnist_amd.engine.graphstep import GraphedStep
    t, ds = make_trainer(data_dir, tmp_path / "s", "--device_data")
    t.attach_dataset(ds)
    g = GraphedStep(t, (BATCH, 28, 28, 1), split=True, dataset=ds)
    assert g.two_graph and g.ds is ds
    t._graph, t._graph_tried = g, True
    loss = None
    for step in range(9):
        _, loss, _, _ = t.resident_step()
        ex, ey = ds.batch_at(step, BATCH)
        assert torch.equal(bits(g.static_x), bits(ex)), step
        assert torch.equal(g.static_y, ey), step
    assert t.step == 9 and int(g.step_dev.item()) == 9
    loss_s = float(loss)
    loss_e, _ = run_resident(data_dir, tmp_path / "e", 9,
                             "--hip_graph", "off")
    print(f"split-graph-resident loss {loss_s:.6f} eager-resident "
          f"{loss_e:.6f} delta {abs(loss_s - loss_e):.3e}")
    assert abs(loss_s - loss_e) < 0.05 * max(1.0, abs(loss_e)), \
        (loss_s, loss_e)
