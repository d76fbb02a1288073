"""pool2 backward fused into its consumers: fc1 dX writes the pooled gradient
gp [B,7,7,64] (linear_dx_pooled) and conv2 dX / dW rebuild the dense pre-pool
gradient in LDS from (gp, am) (conv_dx_pooled, conv_dw_pooled_into).  Each op
is held against the dense-dact op it replaces in the fused step, the dW also
against the fp64 unfold + bmm reference of test_conv2_dw_slab_gpu.py.

Inputs: gp dense with |v| in [0.25, 0.75) and random sign, am drawn from
{0,1,2,3,7} with every value present (plus a case holding 4, 6 and 255), x
dense with non-zero borders.  The dense dact of the references is the torch
scatter of (gp, am).
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
H = W = 14
HO = WO = 7
CIN, COUT = 32, 64
NOUT = 25 * CIN * COUT


@pytest.fixture(scope="module")
def ext():
    from distributedmnist_amd import _C
    m = _C.ext()
    assert m is not None, "HIP extension must be present on GPU boxes"
    return m


@pytest.fixture(autouse=True)
def _default_dispatch(monkeypatch):
    for k in ("DMNIST_DW2_SLAB", "DMNIST_DW2_G", "DMNIST_DW2_KHB",
              "DMNIST_DW2_NBUF", "DMNIST_DW_G", "DMNIST_DW_SPREAD",
              "DMNIST_UNPOOL_LINES", "DMNIST_UNPOOL_TILE", "DMNIST_DX_PAIR",
              "DMNIST_DX_HIOCC", "DMNIST_DX_DB2SLIM", "DMNIST_POOL2_FUSED",
              "DMNIST_OVERLAP", "DMNIST_TWO_STREAM", "DMNIST_SINGLE_STREAM"):
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
    flat = am.view(-1)
    flat[:len(values)] = choice            # every value present
    return am


def scatter(gp, am):
    """Dense dact [NB,14,14,64] of (gp, am): the value at the window position
    the byte names, nothing for any byte outside 0..3."""
    nb = gp.shape[0]
    dact = torch.zeros((nb, H, W, COUT), device="cuda", dtype=bf16)
    for pos in range(4):
        rr, cc = pos >> 1, pos & 1
        dact[:, rr::2, cc::2, :] = torch.where(am == pos, gp,
                                               torch.zeros_like(gp))
    return dact


def gather(dact, am):
    """The (gp, am) gather of a dense dact: inverse of scatter on live
    windows, zero on dead ones."""
    gp = torch.zeros(am.shape, device="cuda", dtype=bf16)
    for pos in range(4):
        rr, cc = pos >> 1, pos & 1
        gp = torch.where(am == pos, dact[:, rr::2, cc::2, :], gp)
    return gp


_CASES = {}


def case(nb):
    """(x, gp, am, dact, fp64 dW reference) for one batch size, once."""
    if nb not in _CASES:
        gen = torch.Generator(device="cuda").manual_seed(5000 + nb)
        x = signed((nb, H, W, CIN), gen)
        gp = signed((nb, HO, WO, COUT), gen)
        am = draw_am((nb, HO, WO, COUT), gen)
        dact = scatter(gp, am)
        _CASES[nb] = (x, gp, am, dact, ref_fp64(x, dact))
    return _CASES[nb]


def ref_fp64(x, dact):
    nb = x.shape[0]
    dw = torch.zeros((CIN * 25, COUT), device="cuda", dtype=torch.float64)
    for i in range(0, nb, 512):
        patches = F.unfold(x[i:i + 512].double().permute(0, 3, 1, 2),
                           kernel_size=5, padding=2)    # [n, ci*25, 196]
        d = dact[i:i + 512].double().reshape(-1, H * W, COUT)
        dw += torch.bmm(patches, d).sum(dim=0)
    return dw.view(CIN, 25, COUT).permute(1, 0, 2).reshape(NOUT)


def check(tag, dw, ref, mult=1.0):
    """Tolerance of test_conv2_dw_slab_gpu.py."""
    ref = ref.float() * mult
    scale = float(ref.abs().max())
    print(f"{tag}: max err={float((dw - ref).abs().max()):.3e} "
          f"(scale {scale:.3e})")
    torch.testing.assert_close(dw, ref, rtol=1e-2,
                               atol=1e-3 * max(scale, 1.0))


def poison(shape, dtype):
    """NaN-fill and free a block of the output's size: the caching allocator
    hands it to the next same-size torch.empty, so an element the kernel
    leaves unwritten shows up as NaN."""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.fill_(float("nan"))
    torch.cuda.synchronize()
    del t


# ---------------------------------------------------------------------------
# 1. producer
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("B", [1, 65, 129])
def test_producer_matches_unpool(ext, B, hidden, tile):
    gen = torch.Generator(device="cuda").manual_seed(B * 1000 + hidden)
    K = HO * WO * COUT
    dyeff = (torch.randn((B, hidden), device="cuda", generator=gen)
             * 0.1).to(bf16)
    w = (torch.randn((K, hidden), device="cuda", generator=gen)
         * 0.05).to(bf16)
    am = draw_am((B, HO, WO, COUT), gen)

    db_ref = torch.zeros(COUT, device="cuda")
    dact = ext.linear_dx_unpool(dyeff, w, am, db_ref, HO, WO, COUT)
    db = torch.zeros(COUT, device="cuda")
    poison((B, HO, WO, COUT), bf16)
    gp = ext.linear_dx_pooled(dyeff, w, am, db, HO, WO, COUT, tile=tile)
    torch.cuda.synchronize()

    assert gp.shape == (B, HO, WO, COUT)
    assert not torch.isnan(gp.float()).any()
    want = gather(dact, am)
    assert torch.equal(gp.view(torch.int16), want.view(torch.int16))
    dead = am >= 4
    assert bool(dead.any())
    assert bool((gp.view(torch.int16)[dead] == 0).all())   # +0, not -0

    # db: the bias-grad bound of test_fc1_epilogues_gpu.py — both kernels sum
    # the same fp32 terms in another order
    gref = (dyeff.float() @ w.float().t()).view(B, HO, WO, COUT) * (am < 4)
    sum_abs = gref.abs().sum(dim=(0, 1, 2))
    bound = 2.0 * (B * HO * WO) * 2.0 ** -24 * sum_abs
    diff = (db - db_ref).abs()
    print("db pooled-vs-unpool max diff", float(diff.max()), "bound min",
          float(bound.min()))
    assert bool((diff <= bound).all())
    # accumulates: a second call doubles it (up to the same reordering)
    ext.linear_dx_pooled(dyeff, w, am, db, HO, WO, COUT, tile=tile)
    diff2 = (db - 2.0 * db_ref).abs()
    assert bool((diff2 <= 2.0 * bound).all())


def test_producer_default_tile_is_one_of_the_two(ext):
    picks = {int(ext.linear_dx_pooled_tile(b, HO * WO * COUT))
             for b in (1, 1024, 65536)}
    assert picks <= {64, 128} and 64 in picks


# ---------------------------------------------------------------------------
# 2. conv2 dX
# ---------------------------------------------------------------------------
def conv_w(seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn((5, 5, CIN, COUT), device="cuda", generator=gen)
            * 0.05).to(bf16)


@pytest.mark.parametrize("force_db", [2, 1])
@pytest.mark.parametrize("nb", [1, 3])
def test_dx_bitwise(ext, nb, force_db):
    _, gp, am, dact, _ = case(nb)
    w = conv_w(91)
    ref = ext.conv_dx(dact, w, CIN)      # NB < 2048: the DB=2 kernel
    poison((nb, H, W, CIN), bf16)
    dx = ext.conv_dx_pooled(gp, am, w, CIN, force_db=force_db)
    torch.cuda.synchronize()
    assert dx.shape == ref.shape
    assert not torch.isnan(dx.float()).any()
    assert bool((ref != 0).any())
    # DB only changes how the weight tile is staged: the sum order is shared
    assert torch.equal(dx.view(torch.int16), ref.view(torch.int16))
    # default dispatch
    dx0 = ext.conv_dx_pooled(gp, am, w, CIN)
    assert torch.equal(dx0.view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("force_db", [2, 1])
def test_dx_ignores_gp_at_dead_windows(ext, force_db):
    nb = 3
    _, gp, am, dact, _ = case(nb)       # gp is non-zero at the dead windows
    assert bool((gp[am == 7] != 0).all())
    w = conv_w(92)
    ref = ext.conv_dx(dact, w, CIN)     # dact has them zeroed
    dx = ext.conv_dx_pooled(gp, am, w, CIN, force_db=force_db)
    assert torch.equal(dx.view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("force_db", [2, 1])
def test_dx_odd_am_bytes(ext, force_db):
    nb = 3
    gen = torch.Generator(device="cuda").manual_seed(93)
    gp = signed((nb, HO, WO, COUT), gen)
    am = draw_am((nb, HO, WO, COUT), gen, values=(0, 1, 2, 3, 7, 4, 6, 255))
    for v in (4, 6, 255):
        assert bool((am == v).any())
    dact = scatter(gp, am)              # 4, 6, 255 scatter nothing
    w = conv_w(94)
    ref = ext.conv_dx(dact, w, CIN)
    dx = ext.conv_dx_pooled(gp, am, w, CIN, force_db=force_db)
    assert torch.equal(dx.view(torch.int16), ref.view(torch.int16))


# ---------------------------------------------------------------------------
# 3. conv2 dW
# ---------------------------------------------------------------------------
def tiers(ext):
    first = {}
    for nb in range(1, 16385):
        first.setdefault(int(ext.conv2_dw_group(nb)), nb)
    return first


def batches(ext):
    """NB=1, then the smallest NB + 1 of every images-per-block tier."""
    return sorted({1} | {n + 1 for n in tiers(ext).values()})


def grouped_nb(ext):
    t = tiers(ext)
    g = min(k for k in t if k > 1)
    return t[g] + 1, g


def run_dw(ext, x, gp, am, dw=None):
    if dw is None:
        dw = torch.zeros(NOUT, device="cuda")
    ext.conv_dw_pooled_into(x, gp, am, dw)
    return dw


def test_dw_values(ext):
    for nb in batches(ext):
        x, gp, am, dact, ref = case(nb)
        tag = f"NB={nb} G={int(ext.conv2_dw_group(nb))}"
        dw = run_dw(ext, x, gp, am)
        check(tag + " vs fp64", dw, ref)
        dense = torch.zeros(NOUT, device="cuda")
        ext.conv_dw_into(x, dact, dense)
        check(tag + " vs conv_dw_into", dw, dense)
        run_dw(ext, x, gp, am, dw)
        check(tag + " second call", dw, ref, mult=2.0)


def test_dw_odd_am_bytes(ext):
    nb = 3
    gen = torch.Generator(device="cuda").manual_seed(95)
    x = signed((nb, H, W, CIN), gen)
    gp = signed((nb, HO, WO, COUT), gen)
    am = draw_am((nb, HO, WO, COUT), gen, values=(0, 1, 2, 3, 7, 4, 6, 255))
    check("odd am bytes", run_dw(ext, x, gp, am),
          ref_fp64(x, scatter(gp, am)))


def _only(t, img):
    out = torch.zeros_like(t)
    out[img] = t[img]
    return out


def test_dw_zero_across_images(ext):
    """x lives in image i only, gp in image i+1 only (and the reverse): a
    stale D row, a stale pad column or a wrong image in the per-block loop
    would pair them.  am stays dense so every window of the gp image is
    decoded."""
    nb, g = grouped_nb(ext)
    x, gp, am, _, _ = case(nb)
    for i in sorted({0, 1, g - 2, g - 1, g, nb - 2} & set(range(nb - 1))):
        dw = run_dw(ext, _only(x, i), _only(gp, i + 1), am)
        assert bool((dw == 0).all()), (nb, g, i, "x before gp")
        dw = run_dw(ext, _only(x, i + 1), _only(gp, i), am)
        assert bool((dw == 0).all()), (nb, g, i, "gp before x")


# ---------------------------------------------------------------------------
# 4. the fused step
# ---------------------------------------------------------------------------
STEP_B = 64


def _step_grads(monkeypatch, fused: str, graph: bool, tag: str):
    """One FusedLeNetStep fwd+bwd at B=64 from the seed's initial weights
    (no update is applied): (loss, acc, {name: grad})."""
    from distributedmnist_amd.engine.fused_step import FusedLeNetStep
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    monkeypatch.setenv("DMNIST_POOL2_FUSED", fused)
    flags = build_train_parser().parse_args(
        ["--synthetic_data", "--train_dir", f"/tmp/dmp2_{tag}",
         "--batch_size", str(STEP_B), "--max_steps", "1", "--model", "lenet",
         "--save_interval_secs", "100000", "--hip_graph", "off"])
    t = Trainer(flags, device=torch.device("cuda:0"))
    ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
    x, y = ds.next_batch(STEP_B)
    step = FusedLeNetStep(t)
    step.overlap_allreduce = False
    assert step.pool2_fused == (fused == "1")
    step_dev = torch.zeros(1, dtype=torch.int64, device=t.device)
    fp = t.fp
    fp.flat_grad.zero_()
    if not graph:
        loss, acc = step(x, y, step_dev)
    else:
        step(x, y, step_dev)              # warm up outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                loss, acc = step(x, y, step_dev)
        torch.cuda.current_stream().wait_stream(s)
        fp.flat_grad.zero_()
        g.replay()
    torch.cuda.synchronize()
    grads = {n: fp.flat_grad[o:o + k].clone()
             for n, o, k in zip(fp.names, fp.offsets, fp.numels)}
    return loss.clone(), acc.clone(), grads


@pytest.fixture(scope="module")
def dense_steps():
    """The DMNIST_POOL2_FUSED=0 step twice: the reference and its own
    run-to-run noise (fp32 atomic order)."""
    mp = pytest.MonkeyPatch()
    try:
        a = _step_grads(mp, "0", False, "d1")
        b = _step_grads(mp, "0", False, "d2")
    finally:
        mp.undo()
    return a, b


@pytest.mark.parametrize("graph", [False, True])
def test_step_matches_dense_route(ext, dense_steps, monkeypatch, graph):
    (loss0, acc0, g0), (_, _, g0b) = dense_steps
    loss1, acc1, g1 = _step_grads(monkeypatch, "1", graph, f"f{int(graph)}")
    assert torch.equal(loss1, loss0) and torch.equal(acc1, acc0)
    # the noise bound of test_ops_gpu.py::test_graphed_step_matches_eager
    for name in ("conv1_w", "conv1_b", "conv2_b"):
        noise = float((g0[name] - g0b[name]).abs().max())
        diff = float((g1[name] - g0[name]).abs().max())
        print(f"{name}: fused-vs-dense {diff:.3e}, dense-vs-dense "
              f"{noise:.3e}")
        assert diff < max(10 * noise, 0.02), (name, diff, noise)
        assert bool((g0[name] != 0).any())
    check("conv2_w fused-vs-dense", g1["conv2_w"], g0["conv2_w"])
    assert bool((g0["conv2_w"] != 0).any())
