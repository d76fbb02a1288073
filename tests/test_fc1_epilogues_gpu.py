"""fc1 epilogues: the line-store unpool epilogue of the dX GEMM, the planned
(single-writer / clamped split-K) dW, and the in-kernel split-K forward
fix-up (DMNIST_FC_FIXUP=1; built and kept bit-identical, not dispatched by
default), each against the path it replaces or an fp64 reference."""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
SWITCHES = ("DMNIST_UNPOOL_LINES", "DMNIST_UNPOOL_TILE", "DMNIST_DW_PLAN",
            "DMNIST_FC_FIXUP")


@pytest.fixture(scope="module")
def ext():
    from distributedmnist_amd import _C
    m = _C.ext()
    assert m is not None, "HIP extension must be present on GPU boxes"
    return m


@pytest.fixture(autouse=True)
def clear_switches():
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def poison(shape, dtype):
    """Allocate, NaN-fill and free a block of the output's size: the caching
    allocator hands it to the next same-size torch.empty, so any element the
    kernel leaves unwritten shows up as NaN."""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.fill_(float("nan"))
    torch.cuda.synchronize()
    del t


# ---------------------------------------------------------------------------
# dX + unpool
# ---------------------------------------------------------------------------
UNPOOL_CASES = [
    (1, 7, 7, 64, 64, None),
    (65, 7, 7, 64, 136, None),
    (3, 2, 3, 64, 64, None),
    (3, 4, 4, 32, 64, None),     # C % 64 != 0: the per-element route
    (3, 2, 2, 128, 64, None),
    # one full 128-row tile plus one row; last column tile half outside N
    (129, 7, 7, 64, 64, "128"),
]


@pytest.mark.parametrize("B,Ho,Wo,C,hidden,tile", UNPOOL_CASES)
def test_unpool_lines_match_element_stores(ext, B, Ho, Wo, C, hidden, tile):
    g = torch.Generator().manual_seed(B * 1000 + Ho * 100 + C + hidden)
    K = Ho * Wo * C
    dyeff = (torch.randn(B, hidden, generator=g) * 0.1).to(bf16).cuda()
    w = (torch.randn(K, hidden, generator=g) * 0.05).to(bf16).cuda()
    choice = torch.tensor([0, 1, 2, 3, 7, 7, 0, 1], dtype=torch.uint8)
    # 2 of 8 draws are 7: about a quarter of the windows are dead
    amax = choice[torch.randint(0, 8, (B, Ho, Wo, C), generator=g)].cuda()
    if tile:
        os.environ["DMNIST_UNPOOL_TILE"] = tile
    shape = (B, 2 * Ho, 2 * Wo, C)

    os.environ["DMNIST_UNPOOL_LINES"] = "0"
    db_old = torch.zeros(C, device="cuda")
    poison(shape, bf16)
    dact_old = ext.linear_dx_unpool(dyeff, w, amax, db_old, Ho, Wo, C)
    torch.cuda.synchronize()
    del os.environ["DMNIST_UNPOOL_LINES"]
    db_new = torch.zeros(C, device="cuda")
    poison(shape, bf16)
    dact_new = ext.linear_dx_unpool(dyeff, w, amax, db_new, Ho, Wo, C)
    torch.cuda.synchronize()

    assert dact_new.shape == shape
    assert not torch.isnan(dact_old.float()).any()
    assert not torch.isnan(dact_new.float()).any()
    assert torch.equal(dact_new.view(torch.int16), dact_old.view(torch.int16))

    # db: both paths sum the same fp32 terms in another order
    gref = (dyeff.float() @ w.float().t()).view(B, Ho, Wo, C)
    gref = gref * (amax < 4)
    sum_abs = gref.abs().sum(dim=(0, 1, 2))
    n = B * Ho * Wo
    bound = 2.0 * n * 2.0 ** -24 * sum_abs
    diff = (db_new - db_old).abs()
    print("db new-vs-old max diff", float(diff.max()), "bound min",
          float(bound.min()))
    assert bool((diff <= bound).all())
    db_torch = gref.sum(dim=(0, 1, 2))
    scale = float(db_torch.abs().max().clamp(min=1.0))
    torch.testing.assert_close(db_new, db_torch, rtol=2e-2, atol=0.02 * scale)


# ---------------------------------------------------------------------------
# dW
# ---------------------------------------------------------------------------
DW_SHAPES = [(8, 64, 1), (136, 64, 31), (136, 128, 64), (200, 192, 65),
             (136, 128, 130), (3136, 512, 100)]
DW_PLANS = [None, "0", "64,64,1", "64,128,1", "128,64,1", "128,128,1",
            "64,64,2", "128,128,4"]


def empty_slice_free(splitk, B):
    ksteps = -(-B // 64)
    return (splitk - 1) * -(-ksteps // splitk) < ksteps


@pytest.mark.parametrize("plan", DW_PLANS)
@pytest.mark.parametrize("K,N,B", DW_SHAPES)
def test_dw_accumulates_within_fp32_bound(ext, K, N, B, plan):
    g = torch.Generator().manual_seed(K * 7 + N * 3 + B)
    x = torch.randn(B, K, generator=g).to(bf16).cuda()
    dy = (torch.randn(B, N, generator=g) * 0.1).to(bf16).cuda()
    prefill = torch.randn(K, N, generator=g).cuda()
    if plan is not None:
        os.environ["DMNIST_DW_PLAN"] = plan
    tbm, bn, sk = ext.linear_dw_plan(K, N, B)
    assert empty_slice_free(sk, B)
    dw = prefill.clone()
    ext.linear_dw_into(x, dy, dw)
    ref = prefill.double() + x.double().t() @ dy.double()
    mag = x.float().abs().t() @ dy.float().abs() + prefill.abs()
    bound = 8.0 * (B + 8) * 2.0 ** -24 * mag.double()
    err = (dw.double() - ref).abs()
    print("plan", (tbm, bn, sk), "max err/bound", float((err / bound).max()))
    assert bool((err <= bound).all())
    if sk == 1:
        # single-writer: one lane adds each element once, in a fixed k order
        dw2 = prefill.clone()
        ext.linear_dw_into(x, dy, dw2)
        assert torch.equal(dw.view(torch.int32), dw2.view(torch.int32))


@pytest.mark.parametrize("plan", [None, "0"])
def test_dw_plan_never_launches_an_empty_slice(ext, plan):
    if plan is not None:
        os.environ["DMNIST_DW_PLAN"] = plan
    # the listed shapes plus fc2's (N % 64 != 0: the scatter-staged route)
    for K, N in [(k, n) for k, n, _ in DW_SHAPES] + [(512, 10)]:
        for B in range(1, 16385):
            tbm, bn, sk = ext.linear_dw_plan(K, N, B)
            assert sk >= 1 and empty_slice_free(sk, B), (K, N, B, tbm, bn, sk)


# ---------------------------------------------------------------------------
# split-K forward fix-up
# ---------------------------------------------------------------------------
FWD_SHAPES = [(1, 1024, 64), (65, 1032, 72), (130, 3136, 64)]


def fwd_inputs(M, K, N):
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g).to(bf16).cuda()
    w = (torch.randn(K, N, generator=g) * 0.05).to(bf16).cuda()
    b = torch.randn(N, generator=g).cuda()
    return x, w, b, w.t().contiguous()


def fwd_call(ext, inp, relu, use_wt, dev, fixup="1"):
    """One split-K forward, by default through the in-kernel fix-up (the
    launcher does not dispatch it by itself)."""
    os.environ["DMNIST_FC_FIXUP"] = fixup
    x, w, b, wT = inp
    wt = wT if use_wt else None
    if dev is not None:
        return ext.linear_act_fwd_dev(x, w, b, True, 0.5, 1234, dev, wt)
    return ext.linear_act_fwd(x, w, b, relu, 1.0, 0, 0, wt)


@pytest.fixture(scope="module")
def fwd_reference(ext):
    """Two-launch outputs, computed once per configuration."""
    cache = {}

    def get(shape, relu, use_wt, drop):
        key = (shape, relu, use_wt, drop)
        if key not in cache:
            dev = torch.tensor([77], device="cuda") if drop else None
            cache[key] = fwd_call(ext, fwd_inputs(*shape), relu, use_wt, dev,
                                  fixup="0")
            torch.cuda.synchronize()
        return cache[key]
    return get


def bits(t):
    return t.view(torch.int16)


# (relu, dropout): the dropout epilogue exists only with relu
FWD_MODES = [(False, False), (True, False), (True, True)]


@pytest.mark.parametrize("use_wt", [False, True])
@pytest.mark.parametrize("relu,drop", FWD_MODES)
@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_fwd_fixup_matches_two_launch(ext, fwd_reference, shape, relu, drop,
                                      use_wt):
    dev = torch.tensor([77], device="cuda") if drop else None
    inp = fwd_inputs(*shape)
    ref = fwd_reference(shape, relu, use_wt, drop)
    other = FWD_SHAPES[(FWD_SHAPES.index(shape) + 1) % len(FWD_SHAPES)]
    other_ref = fwd_reference(other, relu, use_wt, drop)
    # three calls in a row, then another shape: tickets reset, workspace reused
    for _ in range(3):
        poison(ref.shape, bf16)
        y = fwd_call(ext, inp, relu, use_wt, dev)
        assert torch.equal(bits(y), bits(ref))
    y2 = fwd_call(ext, fwd_inputs(*other), relu, use_wt, dev)
    assert torch.equal(bits(y2), bits(other_ref))
    y = fwd_call(ext, inp, relu, use_wt, dev)
    assert torch.equal(bits(y), bits(ref))


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_fwd_fixup_under_graph_replay(ext, fwd_reference, shape, drop):
    dev = torch.tensor([77], device="cuda") if drop else None
    inp = fwd_inputs(*shape)
    ref = fwd_reference(shape, True, True, drop)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fwd_call(ext, inp, True, True, dev)  # eager warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = fwd_call(ext, inp, True, True, dev)
    for _ in range(3):
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(y), bits(ref))
