"""Weight-resident persistent conv2 kernels (csrc/conv2_resident.hip): one
block per CU keeps the conv2 weights in LDS and walks images.  Both are held
bitwise to the per-image slab kernels they replace — conv_dx_pooled(force_db=3)
to force_db=2 and to the dense conv_dx of the scattered dact, conv_pool_fwd to
its DMNIST_CONV2_RESIDENT=0 route — over batch sizes and grid caps that cover
one block walking every image, uneven splits (5 over 2, 7 over 3) and more
blocks than images.

Inputs follow test_pool2_bwd_fused_gpu.py: signed values with |v| in
[0.25, 0.75), am drawn from {0,1,2,3,7} with every value present.  Every output
is allocated right after a NaN-filled block of its size is freed, so an element
a kernel leaves unwritten, or an LDS read of bytes nobody wrote, shows as NaN.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
H = W = 14
HO = WO = 7
CIN, COUT = 32, 64

NBS = [1, 2, 5, 7]
CAPS = [1, 2, 3, None]
SWITCHES = ("DMNIST_CONV2_RESIDENT", "DMNIST_CONV2_RES_BLOCKS",
            "DMNIST_CONV2_RES_MIN_NB", "DMNIST_CONV2_RES_WAVES",
            "DMNIST_CONV2_RES_PF",
            "DMNIST_DX_PAIR", "DMNIST_DX_HIOCC", "DMNIST_DX_DB2SLIM",
            "DMNIST_POOL2_FUSED", "DMNIST_OVERLAP", "DMNIST_TWO_STREAM",
            "DMNIST_SINGLE_STREAM")


@pytest.fixture(scope="module")
def ext():
    from distributedmnist_amd import _C
    m = _C.ext()
    assert m is not None, "HIP extension must be present on GPU boxes"
    return m


@pytest.fixture(autouse=True)
def _default_dispatch(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def signed(shape, gen):
    """|v| in [0.25, 0.75), random sign, bf16."""
    mag = 0.25 + 0.5 * torch.rand(shape, device="cuda", generator=gen)
    sgn = torch.where(torch.rand(shape, device="cuda", generator=gen) < 0.5,
                      -1.0, 1.0)
    return (mag * sgn).to(bf16)


def draw_am(shape, gen, values=(0, 1, 2, 3, 7)):
    choice = torch.tensor(values, dtype=torch.uint8, device="cuda")
    idx = torch.randint(0, len(values), shape, device="cuda", generator=gen)
    am = choice[idx]
    am.view(-1)[:len(values)] = choice       # every value present
    return am


def scatter(gp, am):
    """Dense dact [NB,14,14,64] of (gp, am)."""
    dact = torch.zeros((gp.shape[0], H, W, COUT), device="cuda", dtype=bf16)
    for pos in range(4):
        rr, cc = pos >> 1, pos & 1
        dact[:, rr::2, cc::2, :] = torch.where(am == pos, gp,
                                               torch.zeros_like(gp))
    return dact


def conv_w(seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn((5, 5, CIN, COUT), device="cuda", generator=gen)
            * 0.05).to(bf16)


def poison(shape, dtype=bf16):
    """NaN-pattern (bf16 0xffff / byte 0xff) a block of the output's size and
    free it: the caching allocator hands it to the next same-size empty()."""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(0xff)
    torch.cuda.synchronize()
    del t


def same(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def set_cap(monkeypatch, cap):
    if cap is None:
        monkeypatch.delenv("DMNIST_CONV2_RES_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("DMNIST_CONV2_RES_BLOCKS", str(cap))


# ---------------------------------------------------------------------------
# dX
# ---------------------------------------------------------------------------
_DX = {}


def dx_case(nb, values=(0, 1, 2, 3, 7)):
    """(gp, am, w, force_db=2 result, dense conv_dx result), once per case."""
    key = (nb, values)
    if key not in _DX:
        from distributedmnist_amd import _C
        e = _C.ext()
        gen = torch.Generator(device="cuda").manual_seed(7000 + nb + len(values))
        gp = signed((nb, HO, WO, COUT), gen)
        am = draw_am((nb, HO, WO, COUT), gen, values)
        w = conv_w(191)
        _DX[key] = (gp, am, w, e.conv_dx_pooled(gp, am, w, CIN, force_db=2),
                    e.conv_dx(scatter(gp, am), w, CIN))
    return _DX[key]


def run_dx(ext, gp, am, w):
    poison((gp.shape[0], H, W, CIN))
    dx = ext.conv_dx_pooled(gp, am, w, CIN, force_db=3)
    torch.cuda.synchronize()
    assert dx.shape == (gp.shape[0], H, W, CIN)
    assert not torch.isnan(dx.float()).any()
    return dx


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("nb", NBS)
def test_dx_bitwise(ext, monkeypatch, nb, cap):
    gp, am, w, ref2, dense = dx_case(nb)
    set_cap(monkeypatch, cap)
    dx = run_dx(ext, gp, am, w)
    assert bool((dense != 0).any())
    assert same(dx, ref2)
    assert same(dx, dense)


@pytest.mark.parametrize("variant", [(4, 0), (4, 1), (8, 0), (8, 1)])
def test_dx_variants_bitwise(ext, monkeypatch, variant):
    """The wave-count and prefetch switches change no bit."""
    waves, pf = variant
    monkeypatch.setenv("DMNIST_CONV2_RES_WAVES", str(waves))
    monkeypatch.setenv("DMNIST_CONV2_RES_PF", str(pf))
    gp, am, w, ref2, dense = dx_case(7)
    set_cap(monkeypatch, 3)
    assert same(run_dx(ext, gp, am, w), dense)


def test_dx_odd_am_bytes(ext, monkeypatch):
    values = (0, 1, 2, 3, 7, 4, 6, 255)
    gp, am, w, ref2, dense = dx_case(5, values)
    for v in (4, 6, 255):
        assert bool((am == v).any())
    set_cap(monkeypatch, 2)
    dx = run_dx(ext, gp, am, w)
    assert same(dx, ref2) and same(dx, dense)   # 4, 6, 255 scatter nothing


@pytest.mark.parametrize("zero_first", [True, False])
def test_dx_nothing_survives(ext, monkeypatch, zero_first):
    """One block alternates all-zero and dense images: a zero gradient gives
    exactly zero dX, a dense one its own result."""
    nb = 6
    gp, am, w, _, _ = dx_case(7)
    gp = gp[:nb].clone()
    am = am[:nb].contiguous()
    zero = torch.arange(nb, device="cuda") % 2 == (0 if zero_first else 1)
    gp[zero] = 0
    dense = ext.conv_dx(scatter(gp, am), w, CIN)
    set_cap(monkeypatch, 1)
    dx = run_dx(ext, gp, am, w)
    assert bool((dx.view(torch.int16)[zero] == 0).all())     # +0 everywhere
    assert bool((dx[~zero] != 0).any())
    assert same(dx, dense)


# ---------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------
_FW = {}


def fwd_case(nb):
    """(x, w, bias, y, amax of the DMNIST_CONV2_RESIDENT=0 route), once.  The
    bias is strongly negative on a quarter of the channels, so windows there
    are ReLU-dead (byte 7)."""
    if nb not in _FW:
        from distributedmnist_amd import _C
        e = _C.ext()
        gen = torch.Generator(device="cuda").manual_seed(8000 + nb)
        x = signed((nb, H, W, CIN), gen)
        w = conv_w(192)
        bias = torch.randn(COUT, device="cuda", generator=gen) * 0.1
        bias[::4] = -50.0
        mp = pytest.MonkeyPatch()
        try:
            mp.setenv("DMNIST_CONV2_RESIDENT", "0")
            y, a = e.conv_pool_fwd(x, w, bias, None)
            torch.cuda.synchronize()
        finally:
            mp.undo()
        _FW[nb] = (x, w, bias, y, a)
    return _FW[nb]


def run_fwd(ext, monkeypatch, x, w, bias):
    # the forward kernel is off by default: switch it on, at any NB
    monkeypatch.setenv("DMNIST_CONV2_RESIDENT", "fwd")
    monkeypatch.setenv("DMNIST_CONV2_RES_MIN_NB", "1")
    assert ext.conv2_resident_route(0, x.shape[0])
    poison((x.shape[0], HO, WO, COUT))
    poison((x.shape[0], HO, WO, COUT), torch.uint8)
    y, a = ext.conv_pool_fwd(x, w, bias, None)
    torch.cuda.synchronize()
    assert y.shape == a.shape == (x.shape[0], HO, WO, COUT)
    assert not torch.isnan(y.float()).any()
    return y, a


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("nb", NBS)
def test_fwd_bitwise(ext, monkeypatch, nb, cap):
    x, w, bias, y0, a0 = fwd_case(nb)
    assert bool((a0 == 7).any()) and bool((a0 < 4).any())
    set_cap(monkeypatch, cap)
    y, a = run_fwd(ext, monkeypatch, x, w, bias)
    assert same(y, y0)
    assert torch.equal(a, a0)


@pytest.mark.parametrize("variant", [(4, 0), (4, 1), (8, 0), (8, 1)])
def test_fwd_variants_bitwise(ext, monkeypatch, variant):
    waves, pf = variant
    monkeypatch.setenv("DMNIST_CONV2_RES_WAVES", str(waves))
    monkeypatch.setenv("DMNIST_CONV2_RES_PF", str(pf))
    x, w, bias, y0, a0 = fwd_case(7)
    set_cap(monkeypatch, 3)
    y, a = run_fwd(ext, monkeypatch, x, w, bias)
    assert same(y, y0) and torch.equal(a, a0)


@pytest.mark.parametrize("zero_first", [True, False])
def test_fwd_nothing_survives(ext, monkeypatch, zero_first):
    """One block alternates all-zero and dense images: a zero image gives
    exactly maxpool(relu(bias)), a dense one its own result."""
    nb = 6
    x, w, bias, _, _ = fwd_case(7)
    x = x[:nb].clone()
    zero = torch.arange(nb, device="cuda") % 2 == (0 if zero_first else 1)
    x[zero] = 0
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("DMNIST_CONV2_RESIDENT", "0")
        y0, a0 = ext.conv_pool_fwd(x, w, bias, None)
    finally:
        mp.undo()
    set_cap(monkeypatch, 1)
    y, a = run_fwd(ext, monkeypatch, x, w, bias)
    want = torch.relu(bias).to(bf16).expand(HO, WO, COUT)
    for i in torch.nonzero(zero).flatten().tolist():
        assert same(y[i], want.contiguous())
        # the first of four equal values wins; all-zero windows are dead
        assert torch.equal(a[i], torch.where(bias > 0, 0, 7).to(torch.uint8)
                           .expand(HO, WO, COUT))
    assert same(y, y0) and torch.equal(a, a0)


def test_route_switches(ext, monkeypatch):
    """DMNIST_CONV2_RESIDENT=0|fwd|dx|both and the NB tier, decided in one
    place; the default is dX only; unparsable switches raise."""
    big = 1 << 14
    assert not ext.conv2_resident_route(0, big)        # forward: off
    assert ext.conv2_resident_route(1, big)            # dX: on, by NB
    assert not ext.conv2_resident_route(1, 1)
    monkeypatch.setenv("DMNIST_CONV2_RES_MIN_NB", "1")
    assert not ext.conv2_resident_route(0, 1) and ext.conv2_resident_route(1, 1)
    monkeypatch.setenv("DMNIST_CONV2_RESIDENT", "both")
    assert ext.conv2_resident_route(0, 1) and ext.conv2_resident_route(1, 1)
    monkeypatch.setenv("DMNIST_CONV2_RESIDENT", "0")
    assert not ext.conv2_resident_route(0, big)
    assert not ext.conv2_resident_route(1, big)
    monkeypatch.setenv("DMNIST_CONV2_RESIDENT", "fwd")
    assert ext.conv2_resident_route(0, 1) and not ext.conv2_resident_route(1, 1)
    monkeypatch.setenv("DMNIST_CONV2_RESIDENT", "dx")
    assert not ext.conv2_resident_route(0, 1) and ext.conv2_resident_route(1, 1)
    monkeypatch.setenv("DMNIST_CONV2_RESIDENT", "yes")
    with pytest.raises(RuntimeError):
        ext.conv2_resident_route(1, big)
    monkeypatch.setenv("DMNIST_CONV2_RESIDENT", "dx")
    for bad in ("x", "0", "-3", "12q"):
        monkeypatch.setenv("DMNIST_CONV2_RES_MIN_NB", bad)
        with pytest.raises(RuntimeError):
            ext.conv2_resident_route(1, big)


def test_schedule_follows_dx_route(ext, monkeypatch):
    """The fused step takes the single stream at a large batch only where the
    resident dX actually runs: not with it switched off, and not on the dense
    DMNIST_POOL2_FUSED=0 route, which never launches it."""
    from distributedmnist_amd.engine.fused_step import FusedLeNetStep
    from distributedmnist_amd.engine.train import Trainer
    from distributedmnist_amd.utils.flags import build_train_parser
    flags = build_train_parser().parse_args(
        ["--synthetic_data", "--train_dir", "/tmp/dmc2r_sched",
         "--batch_size", "4096", "--max_steps", "1", "--model", "lenet",
         "--save_interval_secs", "100000", "--hip_graph", "off"])
    t = Trainer(flags, device=torch.device("cuda:0"))
    assert FusedLeNetStep(t).overlap_level == 0
    monkeypatch.setenv("DMNIST_CONV2_RESIDENT", "0")
    assert FusedLeNetStep(t).overlap_level == 2
    monkeypatch.setenv("DMNIST_CONV2_RESIDENT", "fwd")
    assert FusedLeNetStep(t).overlap_level == 2
    monkeypatch.delenv("DMNIST_CONV2_RESIDENT")
    monkeypatch.setenv("DMNIST_POOL2_FUSED", "0")
    assert FusedLeNetStep(t).overlap_level == 2


# ---------------------------------------------------------------------------
# the fused step, captured
# ---------------------------------------------------------------------------
def _step_batch(ext):
    """Smallest batch at which the default dispatch takes the resident dX."""
    for nb in range(1, 16385):
        if ext.conv2_resident_route(1, nb):
            return nb
    raise AssertionError("no batch size routes to the resident kernels")


def _step_grads(batch, resident, replays, tag):
    """One FusedLeNetStep fwd+bwd from the seed's initial weights (no update
    is applied): (loss, acc, {name: grad}); with replays > 0 the step is
    captured and each replay's result is returned.  resident: None leaves the
    default dispatch, otherwise the value of DMNIST_CONV2_RESIDENT."""
    from distributedmnist_amd.engine.fused_step import FusedLeNetStep
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    mp = pytest.MonkeyPatch()
    try:
        if resident is not None:
            mp.setenv("DMNIST_CONV2_RESIDENT", resident)
        flags = build_train_parser().parse_args(
            ["--synthetic_data", "--train_dir", f"/tmp/dmc2r_{tag}",
             "--batch_size", str(batch), "--max_steps", "1", "--model",
             "lenet", "--save_interval_secs", "100000", "--hip_graph", "off"])
        t = Trainer(flags, device=torch.device("cuda:0"))
        ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
        x, y = ds.next_batch(batch)
        step = FusedLeNetStep(t)
        step.overlap_allreduce = False
        step_dev = torch.zeros(1, dtype=torch.int64, device=t.device)
        fp = t.fp

        def result(loss, acc):
            torch.cuda.synchronize()
            grads = {n: fp.flat_grad[o:o + k].clone()
                     for n, o, k in zip(fp.names, fp.offsets, fp.numels)}
            return loss.clone(), acc.clone(), grads

        fp.flat_grad.zero_()
        if not replays:
            return [result(*step(x, y, step_dev))]
        step(x, y, step_dev)              # warm up outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                loss, acc = step(x, y, step_dev)
        torch.cuda.current_stream().wait_stream(s)
        out = []
        for _ in range(replays):
            fp.flat_grad.zero_()
            g.replay()
            out.append(result(loss, acc))
        return out
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def slab_steps(ext):
    """The DMNIST_CONV2_RESIDENT=0 step twice, eager: the reference and its
    own run-to-run noise (fp32 atomic order)."""
    batch = _step_batch(ext)
    (a,) = _step_grads(batch, "0", 0, "s1")
    (b,) = _step_grads(batch, "0", 0, "s2")
    return batch, a, b


@pytest.mark.parametrize("resident", [None, "both"])
def test_graphed_step_matches_slab_route(ext, slab_steps, resident):
    """Default dispatch (resident dX), and with the forward kernel switched on
    as well: captured, replayed three times."""
    batch, (loss0, acc0, g0), (_, _, g0b) = slab_steps
    assert ext.conv2_resident_route(1, batch)
    for i, (loss1, acc1, g1) in enumerate(
            _step_grads(batch, resident, 3, f"r{resident}")):
        assert torch.equal(loss1, loss0) and torch.equal(acc1, acc0)
        # the bounds of test_pool2_bwd_fused_gpu.py::test_step_matches_dense_route
        for name in g0:
            noise = float((g0[name] - g0b[name]).abs().max())
            diff = float((g1[name] - g0[name]).abs().max())
            print(f"replay {i} {name}: resident-vs-slab {diff:.3e}, "
                  f"slab-vs-slab {noise:.3e}")
            if name == "conv2_w":
                scale = float(g0[name].abs().max())
                torch.testing.assert_close(g1[name], g0[name], rtol=1e-2,
                                           atol=1e-3 * max(scale, 1.0))
            else:
                assert diff < max(10 * noise, 0.02), (i, name, diff, noise)
        assert bool((g0["conv2_w"] != 0).any())
        assert bool((g0["conv1_w"] != 0).any())
