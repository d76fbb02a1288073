"""LeNet conv2 dW from pixel-major LDS slabs (csrc/conv2_dw_slab.hip).

Shapes are 14x14x32 -> 64 throughout.  x is dense with |x| in [0.25, 0.75)
and random sign (non-zero borders), dact is dense randn*0.1 — not pool-
sparse — so halo and row-wrap errors cannot hide in structural zeros.  The
reference is fp64 F.unfold + bmm.  The kernel it replaces (conv_dw_tr) is
reached through DMNIST_DW2_SLAB=0, read by the dispatch on every call.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
H = W = 14
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
              "DMNIST_DW2_NBUF",
              "DMNIST_DW_G", "DMNIST_DW_SPREAD"):
        monkeypatch.delenv(k, raising=False)


def tiers(ext):
    """{G: smallest NB selecting it} over the launcher's tiers."""
    first = {}
    for nb in range(1, 16385):
        first.setdefault(int(ext.conv2_dw_group(nb)), nb)
    return first


def batches(ext):
    """NB=1, then for every images-per-block tier the smallest NB selecting
    it plus one (last block partial)."""
    return sorted({1} | {n + 1 for n in tiers(ext).values()})


def grouped_nb(ext):
    """Smallest NB + 1 of the smallest G > 1 tier."""
    t = tiers(ext)
    g = min(k for k in t if k > 1)
    return t[g] + 1, g


_CASES = {}


def case(nb):
    """Inputs and the fp64 reference for one batch size, computed once."""
    if nb not in _CASES:
        gen = torch.Generator(device="cuda").manual_seed(4000 + nb)
        mag = 0.25 + 0.5 * torch.rand((nb, H, W, CIN), device="cuda",
                                      generator=gen)
        sgn = torch.where(torch.rand((nb, H, W, CIN), device="cuda",
                                     generator=gen) < 0.5, -1.0, 1.0)
        x = (mag * sgn).to(bf16)
        dact = (torch.randn((nb, H, W, COUT), device="cuda", generator=gen)
                * 0.1).to(bf16)
        _CASES[nb] = (x, dact, ref_fp64(x, dact))
    return _CASES[nb]


def ref_fp64(x, dact):
    nb = x.shape[0]
    # unfold rows are (ci, kh, kw); the kernel's layout is (kh, kw, ci, co)
    dw = torch.zeros((CIN * 25, COUT), device="cuda", dtype=torch.float64)
    for i in range(0, nb, 512):  # chunked: the patches are 1.25 MB / image
        patches = F.unfold(x[i:i + 512].double().permute(0, 3, 1, 2),
                           kernel_size=5, padding=2)    # [n, ci*25, 196]
        d = dact[i:i + 512].double().reshape(-1, H * W, COUT)
        dw += torch.bmm(patches, d).sum(dim=0)
    return dw.view(CIN, 25, COUT).permute(1, 0, 2).reshape(NOUT)


def run(ext, x, dact, dw=None):
    if dw is None:
        dw = torch.zeros(NOUT, device="cuda")
    ext.conv_dw_into(x, dact, dw)
    return dw


def check(tag, dw, ref, mult=1.0):
    ref = ref.float() * mult
    scale = float(ref.abs().max())
    print(f"{tag}: max err={float((dw - ref).abs().max()):.3e} "
          f"(scale {scale:.3e})")
    torch.testing.assert_close(dw, ref, rtol=1e-2,
                               atol=1e-3 * max(scale, 1.0))


def test_tiers_cover_more_than_one_group(ext):
    assert any(g > 1 for g in tiers(ext))


def test_values_against_fp64(ext):
    for nb in batches(ext):
        x, dact, ref = case(nb)
        tag = f"NB={nb} G={int(ext.conv2_dw_group(nb))}"
        dw = run(ext, x, dact)
        check(tag + " vs fp64", dw, ref)
        # accumulate semantics: a second call into the same buffer doubles
        run(ext, x, dact, dw)
        check(tag + " second call", dw, ref, mult=2.0)


@pytest.mark.parametrize("khb,nbuf", [(1, 1), (1, 2), (5, 1), (5, 2)])
def test_kernel_variants(ext, monkeypatch, khb, nbuf):
    """Every instantiation the launcher can pick (DMNIST_DW2_KHB: kernel
    rows per block, DMNIST_DW2_NBUF: slab buffers), whichever is default:
    values, and the image pipeline's exact zero across neighbouring images."""
    monkeypatch.setenv("DMNIST_DW2_KHB", str(khb))
    monkeypatch.setenv("DMNIST_DW2_NBUF", str(nbuf))
    for nb in batches(ext):
        x, dact, ref = case(nb)
        check(f"KHB={khb} NBUF={nbuf} NB={nb}", run(ext, x, dact), ref)
    nb, g = grouped_nb(ext)
    x, dact, _ = case(nb)
    for i in (0, 1, g - 1):
        dw = run(ext, _keep(x, imgs=[i]), _keep(dact, imgs=[i + 1]))
        assert bool((dw == 0).all()), (i, "x before dact")
        dw = run(ext, _keep(x, imgs=[i + 1]), _keep(dact, imgs=[i]))
        assert bool((dw == 0).all()), (i, "dact before x")


def test_conv_pool_bwd_call_site(ext):
    """The dW inside conv_pool_bwd takes the same kernel."""
    nb = 3
    gen = torch.Generator(device="cuda").manual_seed(77)
    x, _, _ = case(nb)
    w = (torch.randn((5, 5, CIN, COUT), device="cuda", generator=gen)
         * 0.05).to(bf16)
    b = torch.zeros(COUT, device="cuda")
    y, am = ext.conv_pool_fwd(x, w, b)
    dy = (torch.randn(y.shape, device="cuda", generator=gen) * 0.1).to(bf16)
    db = torch.zeros(COUT, device="cuda")
    dact = ext.pool_scatter(dy, y, am, db, H, W)
    out = ext.conv_pool_bwd(dy, x, w, y, am, True)
    dw = out[1].reshape(NOUT)
    check("conv_pool_bwd dW vs fp64", dw, ref_fp64(x, dact))


def test_agrees_with_replaced_kernel(ext, monkeypatch):
    for nb in batches(ext):
        x, dact, ref = case(nb)
        dw = run(ext, x, dact)
        monkeypatch.setenv("DMNIST_DW2_SLAB", "0")
        dw_old = run(ext, x, dact)
        monkeypatch.delenv("DMNIST_DW2_SLAB")
        scale = float(ref.abs().max())
        print(f"NB={nb}: max diff vs conv_dw_tr="
              f"{float((dw - dw_old).abs().max()):.3e} (scale {scale:.3e})")
        torch.testing.assert_close(dw, dw_old, rtol=1e-2,
                                   atol=1e-3 * max(scale, 1.0))


def _keep(t, rows=None, cols=None, imgs=None):
    out = torch.zeros_like(t)
    r = slice(None) if rows is None else rows
    c = slice(None) if cols is None else cols
    n = slice(None) if imgs is None else imgs
    out[n, r, c] = t[n, r, c]
    return out


def test_zero_column_wrap(ext):
    # taps reach at most 2 columns: columns {0,1} never meet {12,13}
    for nb in batches(ext):
        x, dact, _ = case(nb)
        dw = run(ext, _keep(x, cols=[0, 1]), _keep(dact, cols=[12, 13]))
        assert bool((dw == 0).all()), nb
        dw = run(ext, _keep(x, cols=[12, 13]), _keep(dact, cols=[0, 1]))
        assert bool((dw == 0).all()), nb


def test_zero_row_halo(ext):
    for nb in batches(ext):
        x, dact, _ = case(nb)
        dw = run(ext, _keep(x, rows=[0, 1]), _keep(dact, rows=[12, 13]))
        assert bool((dw == 0).all()), nb
        dw = run(ext, _keep(x, rows=[12, 13]), _keep(dact, rows=[0, 1]))
        assert bool((dw == 0).all()), nb


def test_zero_across_images(ext):
    # x lives in image i only, dact in image i+1 only: a stale slab or a
    # wrong buffer in the per-block image loop would pair them
    nb, g = grouped_nb(ext)
    x, dact, _ = case(nb)
    for i in sorted({0, 1, g - 2, g - 1, g, nb - 2} & set(range(nb - 1))):
        dw = run(ext, _keep(x, imgs=[i]), _keep(dact, imgs=[i + 1]))
        assert bool((dw == 0).all()), (nb, g, i)
        dw = run(ext, _keep(x, imgs=[i + 1]), _keep(dact, imgs=[i]))
        assert bool((dw == 0).all()), (nb, g, i)


def test_zero_dact(ext):
    for nb in batches(ext):
        x, dact, _ = case(nb)
        dw = run(ext, x, torch.zeros_like(dact))
        assert bool((dw == 0).all()), nb


# (dact pixel, interior x pixel within tap reach of it)
@pytest.mark.parametrize("pix,xpix", [((0, 0), (2, 1)), ((0, 13), (1, 11)),
                                      ((13, 0), (11, 2)), ((13, 13), (12, 12)),
                                      ((6, 7), (6, 9))])
def test_single_tap(ext, pix, xpix):
    """x one-hot at an interior pixel and one ci, dact one-hot at `pix` (the
    four corners and a centre pixel) and one co: exactly one of the 51 200
    outputs is non-zero, at the predicted (kh, kw, ci, co)."""
    nb, _ = grouped_nb(ext)
    (h, w), (xh, xw) = pix, xpix
    kh, kw = xh - h + 2, xw - w + 2
    assert 0 <= kh < 5 and 0 <= kw < 5 and 1 <= xh <= 12 and 1 <= xw <= 12
    for img, ci, co in [(0, 0, 0), (nb - 1, 31, 63), (nb // 2, 17, 42)]:
        x = torch.zeros((nb, H, W, CIN), device="cuda", dtype=bf16)
        dact = torch.zeros((nb, H, W, COUT), device="cuda", dtype=bf16)
        x[img, xh, xw, ci] = 1.5
        dact[img, h, w, co] = 0.5
        dw = run(ext, x, dact)
        nz = torch.nonzero(dw).flatten().tolist()
        want = ((kh * 5 + kw) * CIN + ci) * COUT + co
        assert nz == [want], (pix, img, ci, co, nz, want)
        assert float(dw[want]) == 0.75


def test_graph_replay(ext):
    nb, _ = grouped_nb(ext)
    x, dact, ref = case(nb)
    run(ext, x, dact)  # warm up outside the capture
    dw = torch.zeros(NOUT, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            ext.conv_dw_into(x, dact, dw)
    torch.cuda.current_stream().wait_stream(stream)
    dw.zero_()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    check(f"NB={nb} 3 replays", dw, ref, mult=3.0)
