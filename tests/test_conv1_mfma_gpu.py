"""LeNet conv1 on MFMA (csrc/conv1_mfma.hip): forward and pooled dW/db.

Inputs are dense random bf16 images with non-zero borders — MNIST's blank
margins would hide halo and row-wrap errors.  Shapes are 28x28x1 -> 32.
The v_dot2c kernels the MFMA path replaces are reached through
DMNIST_CONV1_VALU=1 (read by the launcher on every call).
"""

import pytest
import torch
import torch.nn.functional as F

from test_ops_gpu import assert_close_bf16

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16


@pytest.fixture(scope="module")
def ext():
    from distributedmnist_amd import _C
    m = _C.ext()
    assert m is not None, "HIP extension must be present on GPU boxes"
    return m


@pytest.fixture(autouse=True)
def _default_dispatch(monkeypatch):
    monkeypatch.delenv("DMNIST_CONV1_VALU", raising=False)
    monkeypatch.delenv("DMNIST_DW1_G", raising=False)


def dense_images(nb, gen):
    # |x| in [0.25, 0.75): no zero anywhere, borders included
    mag = 0.25 + 0.5 * torch.rand((nb, 28, 28, 1), generator=gen)
    sign = torch.where(torch.rand((nb, 28, 28, 1), generator=gen) < 0.5,
                       -1.0, 1.0)
    return (mag * sign).to(bf16)


_FWD = {}


def fwd_case(nb):
    """Inputs and the fp32 reference for one batch size, computed once."""
    if nb not in _FWD:
        gen = torch.Generator().manual_seed(100 + nb)
        x = dense_images(nb, gen)
        w = (torch.randn((5, 5, 1, 32), generator=gen) * 0.1).to(bf16)
        b = torch.randn(32, generator=gen) * 0.1
        from distributedmnist_amd.ops import cpu_ref
        y_ref, _ = cpu_ref.conv_pool_fwd(x.float(), w.float(), b)
        conv = F.conv2d(x.float().permute(0, 3, 1, 2),
                        w.float().permute(3, 2, 0, 1), b, padding=2)
        act = F.relu(conv)                                  # [N,32,28,28]
        # [N,14,14,32,4] with position = row*2 + col of the 2x2 window
        win = act.view(nb, 32, 14, 2, 14, 2).permute(0, 2, 4, 1, 3, 5)
        win = win.reshape(nb, 14, 14, 32, 4).contiguous()
        _FWD[nb] = dict(x=x.cuda(), w=w.cuda(), b=b.cuda(), y_ref=y_ref,
                        win=win, scale=float(y_ref.abs().max()))
    return _FWD[nb]


@pytest.mark.parametrize("NB", [1, 3, 8])
def test_fwd_values_and_routing(ext, NB):
    c = fwd_case(NB)
    y, am = ext.conv_pool_fwd(c["x"], c["w"], c["b"])
    assert y.shape == (NB, 14, 14, 32) and am.shape == (NB, 14, 14, 32)
    assert am.dtype == torch.uint8
    scale = c["scale"]
    assert_close_bf16(y, c["y_ref"], scale=scale)
    yf, amc, win = y.float().cpu(), am.cpu().long(), c["win"]
    assert set(torch.unique(amc).tolist()) <= {0, 1, 2, 3, 7}
    # dead marker exactly where the pooled output is zero
    assert torch.equal(amc == 7, yf == 0)
    live = amc < 4
    chosen = win.gather(4, amc.clamp(max=3).unsqueeze(-1)).squeeze(-1)
    wmax = win.max(dim=4).values
    # the routed position holds (within fp32 rounding of a 25-term sum) the
    # window maximum, and y is its bf16 rounding — every live window checked
    slack = wmax - chosen
    print(f"NB={NB} live={int(live.sum())} worst routing slack="
          f"{float(slack[live].max()):.3e} bound={1e-4 * scale:.3e}")
    assert bool((slack[live] <= 1e-4 * scale).all())
    assert_close_bf16(yf[live], chosen.to(bf16).float()[live], scale=scale)


def test_fwd_dead_windows(ext):
    c = fwd_case(3)
    b = torch.full((32,), -10.0, device="cuda")
    y, am = ext.conv_pool_fwd(c["x"], c["w"], b)
    assert bool((y == 0).all()) and bool((am == 7).all())


def test_fwd_deterministic(ext):
    c = fwd_case(8)
    y, am = ext.conv_pool_fwd(c["x"], c["w"], c["b"])
    for _ in range(4):
        y2, am2 = ext.conv_pool_fwd(c["x"], c["w"], c["b"])
        assert torch.equal(y, y2) and torch.equal(am, am2)


@pytest.mark.parametrize("NB", [1, 3, 8])
def test_fwd_matches_valu_kernel(ext, NB, monkeypatch):
    c = fwd_case(NB)
    y, am = ext.conv_pool_fwd(c["x"], c["w"], c["b"])
    monkeypatch.setenv("DMNIST_CONV1_VALU", "1")
    y_old, am_old = ext.conv_pool_fwd(c["x"], c["w"], c["b"])
    monkeypatch.delenv("DMNIST_CONV1_VALU")
    # outputs are >= 0, so bf16 bit patterns order like the values: one ulp
    # is a difference of one in the integer view
    ulp = (y.view(torch.int16).int() - y_old.view(torch.int16).int()).abs()
    print(f"NB={NB} max ulp diff={int(ulp.max())} "
          f"differing={int((ulp > 0).sum())}")
    assert int(ulp.max()) <= 1
    diff = (am != am_old).cpu()
    if bool(diff.any()):
        win = c["win"]
        a = win.gather(4, am.cpu().long().clamp(max=3).unsqueeze(-1))
        o = win.gather(4, am_old.cpu().long().clamp(max=3).unsqueeze(-1))
        gap = (a - o).abs().squeeze(-1)[diff]
        print(f"NB={NB} amax differs at {int(diff.sum())}, "
              f"max ref gap={float(gap.max()):.3e}")
        assert bool((gap < 1e-4 * c["scale"]).all())


# ---------------------------------------------------------------------------
# dW / db
# ---------------------------------------------------------------------------

def dw_batches(ext):
    """NB=1, then for every images-per-block tier of the launcher the
    smallest NB selecting it plus one (last block partial)."""
    first = {}
    for nb in range(1, 16385):
        first.setdefault(int(ext.conv1_dw_group(nb)), nb)
    return [1] + sorted(n + 1 for n in first.values())


def dw_inputs(nb, am_mode, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    mag = 0.25 + 0.5 * torch.rand((nb, 28, 28, 1), device="cuda",
                                  generator=gen)
    sgn = torch.where(torch.rand((nb, 28, 28, 1), device="cuda",
                                 generator=gen) < 0.5, -1.0, 1.0)
    x = (mag * sgn).to(bf16)
    dyp = (torch.randn((nb, 14, 14, 32), device="cuda", generator=gen)
           * 0.1).to(bf16)
    if am_mode == "random":
        pos = torch.randint(0, 4, (nb, 14, 14, 32), device="cuda",
                            generator=gen)
        dead = torch.rand((nb, 14, 14, 32), device="cuda",
                          generator=gen) < 0.5
        am = torch.where(dead, torch.full_like(pos, 7), pos)
    else:
        am = torch.full((nb, 14, 14, 32), int(am_mode), device="cuda")
    return x, dyp, am.to(torch.uint8)


def dw_ref_fp64(x, dyp, am):
    nb = x.shape[0]
    gval = torch.where(am < 4, dyp.double(), torch.zeros((), device="cuda",
                                                         dtype=torch.float64))
    g6 = torch.zeros((nb, 14, 2, 14, 2, 32), device="cuda",
                     dtype=torch.float64)
    for pos in range(4):
        g6[:, :, pos >> 1, :, pos & 1, :] = torch.where(
            am == pos, gval, torch.zeros_like(gval))
    g = g6.view(nb, 28, 28, 32)
    # patches [N, 25, 784] (tap = kh*5 + kw) times g [N, 784, 32]
    patches = F.unfold(x.double().view(nb, 1, 28, 28), kernel_size=5,
                       padding=2)
    dw = torch.bmm(patches, g.view(nb, 784, 32)).sum(dim=0)
    return dw.view(800), gval.sum(dim=(0, 1, 2))


def dw_ref_composition(ext, x, dyp, am):
    # pool_scatter masks by y > 0; liveness here lives in the argmax byte
    yp = torch.where(am < 4, 1.0, 0.0).to(bf16)
    db = torch.zeros(32, device="cuda")
    dact = ext.pool_scatter(dyp, yp, am, db, 28, 28)
    dw = torch.zeros(800, device="cuda")
    ext.conv_dw_into(x, dact, dw)
    return dw, db


def check_dw(tag, dw, db, dw_ref, db_ref, mult=1.0):
    dw_ref = dw_ref.float() * mult
    db_ref = db_ref.float() * mult
    scale = float(dw_ref.abs().max())
    print(f"{tag}: dw max err={float((dw - dw_ref).abs().max()):.3e} "
          f"(scale {scale:.3e}) db max err="
          f"{float((db - db_ref).abs().max()):.3e}")
    torch.testing.assert_close(db, db_ref, rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(dw, dw_ref, rtol=1e-2,
                               atol=1e-3 * max(scale, 1.0))


@pytest.mark.parametrize("am_mode", ["random", "0", "1", "2", "3"])
def test_dw_matches_references(ext, am_mode):
    for nb in dw_batches(ext):
        x, dyp, am = dw_inputs(nb, am_mode, 7 * nb + 1)
        dw = torch.zeros(800, device="cuda")
        db = torch.zeros(32, device="cuda")
        ext.conv1_dw_pooled(x, dyp, am, dw, db)
        dw64, db64 = dw_ref_fp64(x, dyp, am)
        dwc, dbc = dw_ref_composition(ext, x, dyp, am)
        tag = f"am={am_mode} NB={nb} G={int(ext.conv1_dw_group(nb))}"
        check_dw(tag + " vs fp64", dw, db, dw64, db64)
        check_dw(tag + " vs composition", dw, db, dwc, dbc)
        # accumulate semantics: a second call into the same buffers doubles
        ext.conv1_dw_pooled(x, dyp, am, dw, db)
        check_dw(tag + " second call", dw, db, dw64, db64, mult=2.0)


def test_dw_all_dead_is_exact_zero(ext):
    for nb in dw_batches(ext):
        x, dyp, am = dw_inputs(nb, "7", 11 * nb + 3)
        dw = torch.zeros(800, device="cuda")
        db = torch.zeros(32, device="cuda")
        ext.conv1_dw_pooled(x, dyp, am, dw, db)
        assert bool((dw == 0).all()) and bool((db == 0).all()), nb


# ---------------------------------------------------------------------------
# softmax-CE: loss/accuracy are stored by the kernel (no zero-fill launch)
# ---------------------------------------------------------------------------

def softmax_case(B):
    gen = torch.Generator().manual_seed(500 + B)
    logits = (torch.randn((B, 10), generator=gen) * 2).to(bf16)
    labels = torch.randint(0, 10, (B,), generator=gen)
    return logits, labels


@pytest.mark.parametrize("B", [1, 255, 257, 1024])
def test_softmax_values_and_no_carry_over(ext, B):
    logits, labels = softmax_case(B)
    from distributedmnist_amd.ops import cpu_ref
    loss_ref, correct_ref, dl_ref = cpu_ref.softmax_xent_fwd(logits.float(),
                                                             labels)
    lg, lb = logits.cuda(), labels.cuda()
    loss, correct, dl = ext.softmax_xent_fwd(lg, lb)
    assert abs(float(loss) - float(loss_ref)) < 0.02 * max(1.0, float(loss_ref))
    assert abs(float(correct) - float(correct_ref)) <= 2  # bf16 argmax ties
    assert_close_bf16(dl, dl_ref, atol=2e-4)
    # a second call returns the same two values: nothing accumulates
    loss2, correct2, _ = ext.softmax_xent_fwd(lg, lb)
    assert float(loss2) == float(loss) and float(correct2) == float(correct)
    # with the fused fc2 bias grad and the accuracy scale as the step uses
    db = torch.zeros(10, device="cuda")
    loss3, acc3, _ = ext.softmax_xent_fwd(lg, lb, db_out=db, inv_n=1.0 / B)
    assert float(loss3) == float(loss)
    assert abs(float(acc3) - float(correct) / B) < 1e-6


@pytest.mark.parametrize("B", [1, 255, 257, 1024])
def test_softmax_graph_replay(ext, B):
    logits, labels = softmax_case(B)
    lg, lb = logits.cuda(), labels.cuda()
    loss, correct, _ = ext.softmax_xent_fwd(lg, lb)   # eager reference
    want = (float(loss), float(correct))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            g_loss, g_correct, _ = ext.softmax_xent_fwd(lg, lb)
    torch.cuda.current_stream().wait_stream(stream)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert (float(g_loss), float(g_correct)) == want
