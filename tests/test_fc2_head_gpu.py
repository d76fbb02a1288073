"""The fused fc2 head (ext.fc2_head: fc2 forward + softmax-xent + fc2 dW +
fc2 dX/mask in one kernel) against the four-launch route of the same build
and the fp64 reference cpu_ref.fc2_head.

Error rule (both routes differ from the reference only in fp32 accumulation
order and the one-ulp bf16 rounding flips that order can cause): the fused
route's maximum absolute error is at most twice the four-launch route's at
the same shape, with a floor of one bf16 ulp of the largest output magnitude
for dyeff1 and of B * 2^-24 times the largest magnitude for the fp32 sums.
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
K, C, P_KEEP = 512, 10, 0.5
SHAPES = [1, 31, 33, 65, 257]
ROWS = [None, 16, 32, 64]
SUMS = ("dw2", "db1", "db2")


@pytest.fixture(scope="module")
def ext():
    from distributedmnist_amd import _C
    m = _C.ext()
    assert m is not None, "HIP extension must be present on GPU boxes"
    return m


@functools.lru_cache(maxsize=None)
def case(B, k=K, c=C):
    """Inputs drawn as tests/test_ops_gpu.py draws them, plus the fp64
    reference of the shape (computed once, never modified)."""
    from distributedmnist_amd.ops import cpu_ref
    gen = torch.Generator().manual_seed(1000 + B + 7 * k + c)
    a1 = torch.randn((B, k), generator=gen).to(bf16).relu()  # ~half zeros
    if B > 1:
        a1[B // 2] = 0  # one all-zero row
    w2 = (torch.randn((k, c), generator=gen) * 0.1).to(bf16)
    b2 = torch.randn((c,), generator=gen) * 0.1
    labels = torch.randint(0, c, (B,), generator=gen)
    labels[0] = c - 1
    if B > 1:
        labels[-1] = 0
    ref = dict(zip(("loss", "correct", "dyeff1", "dw2", "db1", "db2"),
                   cpu_ref.fc2_head(a1, w2, b2, labels, P_KEEP)))
    return dict(a1=a1, w2=w2, b2=b2, labels=labels, ref=ref)


def run(ext, monkeypatch, cs, fused, rows=None, preload=0.0, calls=1,
        inv_n=None):
    """One route of ext.fc2_head on the case; gradients start at `preload`
    and accumulate over `calls` calls.  Returns CPU tensors."""
    monkeypatch.setenv("DMNIST_FC2_FUSED", "1" if fused else "0")
    if rows is None:
        monkeypatch.delenv("DMNIST_FC2_R", raising=False)
    else:
        monkeypatch.setenv("DMNIST_FC2_R", str(rows))
    B, k = cs["a1"].shape
    c = cs["w2"].shape[1]
    a1, w2 = cs["a1"].cuda(), cs["w2"].cuda()
    w2T = w2.t().contiguous()
    b2, labels = cs["b2"].cuda(), cs["labels"].cuda()
    dw2 = torch.full((k, c), preload, device="cuda")
    db2 = torch.full((c,), preload, device="cuda")
    db1 = torch.full((k,), preload, device="cuda")
    for _ in range(calls):
        loss, acc, dyeff1 = ext.fc2_head(
            a1, w2, w2T, b2, labels, dw2, db2, db1, P_KEEP,
            1.0 / B if inv_n is None else inv_n)
    torch.cuda.synchronize()
    return dict(loss=loss.cpu(), acc=acc.cpu(), dyeff1=dyeff1.cpu(),
                dw2=dw2.cpu(), db1=db1.cpu(), db2=db2.cpu())


@functools.lru_cache(maxsize=None)
def _four_cached(ext, B, preload, calls):
    mp = pytest.MonkeyPatch()
    try:
        return run(ext, mp, case(B), False, preload=preload, calls=calls)
    finally:
        mp.undo()


def bf16_ulp(x):
    return 2.0 ** (math.floor(math.log2(x)) - 7) if x > 0 else 0.0


def errors(got, ref, B, offset=0.0, scale=1.0):
    """name -> (max abs error, floor) against scale * ref + offset."""
    out = {}
    want = ref["dyeff1"].double()
    e = float((got["dyeff1"].double() - want).abs().max())
    out["dyeff1"] = (e, bf16_ulp(float(want.abs().max())))
    for name in SUMS:
        want = scale * ref[name] + offset
        e = float((got[name].double() - want).abs().max())
        out[name] = (e, B * 2.0 ** -24 * float(want.abs().max()))
    e = abs(float(got["loss"].double()) - float(ref["loss"]))
    out["loss"] = (e, B * 2.0 ** -24 * abs(float(ref["loss"])))
    return out


def assert_within_twice(fused, four, ref, B, tag, **kw):
    ef, e4 = errors(fused, ref, B, **kw), errors(four, ref, B, **kw)
    for name, (e, floor) in ef.items():
        print(f"{tag} B={B} {name}: fused {e:.3e} four-launch "
              f"{e4[name][0]:.3e} floor {floor:.3e}")
    for name, (e, floor) in ef.items():
        assert e <= max(2.0 * e4[name][0], floor), (tag, B, name, e,
                                                    e4[name][0], floor)


def assert_finite(got):
    for name, t in got.items():
        assert torch.isfinite(t.float()).all(), name


# 1. against the four-launch route, both held to the fp64 reference; 3. the
# accuracy; 5. the all-zero row and finiteness
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("B", SHAPES)
def test_fused_against_four_launch(ext, monkeypatch, B, rows):
    cs = case(B)
    four = _four_cached(ext, B, 0.0, 1)
    fused = run(ext, monkeypatch, cs, True, rows)
    assert_within_twice(fused, four, cs["ref"], B, f"R={rows}")
    assert_finite(fused)
    if B > 1:
        assert not fused["dyeff1"][B // 2].float().any()
    count = run(ext, monkeypatch, cs, True, rows, inv_n=1.0)["acc"]
    assert float(count) == round(float(count))
    assert abs(float(count) - float(cs["ref"]["correct"])) <= 2  # bf16 ties
    if B & (B - 1) == 0:
        assert float(fused["acc"]) == float(count) / B
    else:
        assert abs(float(fused["acc"]) - float(count) / B) < 1e-6


# 2. the bounds the project holds the separate ops to (tests/test_ops_gpu.py)
@pytest.mark.parametrize("rows", ROWS)
def test_project_bounds(ext, monkeypatch, rows):
    B = 257
    cs = case(B)
    ref = cs["ref"]
    got = run(ext, monkeypatch, cs, True, rows, inv_n=1.0)
    loss_ref = float(ref["loss"])
    assert abs(float(got["loss"]) - loss_ref) < 0.02 * max(1.0, loss_ref)
    assert abs(float(got["acc"]) - float(ref["correct"])) <= 2
    want = ref["dyeff1"].float()
    torch.testing.assert_close(got["dyeff1"].float(), want, rtol=0.02,
                               atol=0.02 * float(want.abs().max()))
    for name, floor in (("db1", 1.0), ("db2", 1e-3)):
        want = ref[name].float()
        scale = float(want.abs().max().clamp(min=floor))
        torch.testing.assert_close(got[name], want, rtol=2e-2,
                                   atol=0.02 * scale)


# 4. nothing carries over, and the softmax workspace is shared cleanly
@pytest.mark.parametrize("rows", ROWS)
def test_no_carry_over_and_workspace_sharing(ext, monkeypatch, rows):
    B = 257
    cs = case(B)
    first = run(ext, monkeypatch, cs, True, rows)
    gen = torch.Generator().manual_seed(3)
    lg = (torch.randn((300, C), generator=gen) * 2).to(bf16).cuda()
    lb = torch.randint(0, C, (300,), generator=gen).cuda()
    alone = [float(v) for v in ext.softmax_xent_fwd(lg, lb)[:2]]
    second = run(ext, monkeypatch, cs, True, rows)
    for name in ("loss", "acc"):
        assert torch.equal(first[name], second[name]), name
    after_head = [float(v) for v in ext.softmax_xent_fwd(lg, lb)[:2]]
    assert after_head == alone
    third = run(ext, monkeypatch, cs, True, rows)  # head after a softmax
    for name in ("loss", "acc"):
        assert torch.equal(first[name], third[name]), name


# 5. gradients are accumulated into what the buffers hold
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("B", [33, 257])
def test_accumulate_contract(ext, monkeypatch, B, rows):
    cs = case(B)
    c = 0.25
    four = _four_cached(ext, B, c, 1)
    fused = run(ext, monkeypatch, cs, True, rows, preload=c)
    assert_within_twice(fused, four, cs["ref"], B, f"preload R={rows}",
                        offset=c)
    assert_finite(fused)


# 6. graph replay
@pytest.mark.parametrize("rows", ROWS)
def test_graph_replay(ext, monkeypatch, rows):
    B = 65
    cs = case(B)
    eager = run(ext, monkeypatch, cs, True, rows)
    a1, w2 = cs["a1"].cuda(), cs["w2"].cuda()
    w2T = w2.t().contiguous()
    b2, labels = cs["b2"].cuda(), cs["labels"].cuda()
    dw2 = torch.zeros((K, C), device="cuda")
    db2 = torch.zeros((C,), device="cuda")
    db1 = torch.zeros((K,), device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            g_loss, g_acc, g_dy = ext.fc2_head(a1, w2, w2T, b2, labels, dw2,
                                               db2, db1, P_KEEP, 1.0 / B)
    torch.cuda.current_stream().wait_stream(stream)
    for t in (dw2, db2, db1):
        t.zero_()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_loss.cpu(), eager["loss"])
        assert torch.equal(g_acc.cpu(), eager["acc"])
    assert torch.equal(g_dy.cpu(), eager["dyeff1"])
    got = dict(loss=g_loss.cpu(), dyeff1=g_dy.cpu(), dw2=dw2.cpu(),
               db1=db1.cpu(), db2=db2.cpu())
    four3 = _four_cached(ext, B, 0.0, 3)
    assert_within_twice(got, four3, cs["ref"], B, f"3 replays R={rows}",
                        scale=3.0)


# 7. fallbacks: the op IS the four explicit calls
def four_explicit(ext, cs):
    B, k = cs["a1"].shape
    c = cs["w2"].shape[1]
    a1, w2 = cs["a1"].cuda(), cs["w2"].cuda()
    w2T = w2.t().contiguous()
    b2, labels = cs["b2"].cuda(), cs["labels"].cuda()
    dw2 = torch.zeros((k, c), device="cuda")
    db2 = torch.zeros((c,), device="cuda")
    db1 = torch.zeros((k,), device="cuda")
    logits = ext.linear_act_fwd(a1, w2, b2, False, 1.0, 0, 0, w2T)
    loss, acc, dl = ext.softmax_xent_fwd(logits, labels, db_out=db2,
                                         inv_n=1.0 / B)
    ext.linear_dw_into(a1, dl, dw2)
    dyeff1 = ext.linear_dx_mask(dl, w2, a1, db1, P_KEEP)
    torch.cuda.synchronize()
    return dict(loss=loss.cpu(), acc=acc.cpu(), dyeff1=dyeff1.cpu(),
                dw2=dw2.cpu(), db1=db1.cpu(), db2=db2.cpu())


@pytest.mark.parametrize("k,c", [(512, 7), (96, 10)])
def test_fallback_shapes(ext, monkeypatch, k, c):
    cs = case(65, k, c)
    want = four_explicit(ext, cs)
    got = run(ext, monkeypatch, cs, True)
    assert torch.equal(got["dyeff1"], want["dyeff1"])
    assert torch.equal(got["loss"], want["loss"])


def test_fallback_deterministic(ext, monkeypatch):
    cs = case(257)
    ext.set_deterministic(True)
    try:
        want = four_explicit(ext, cs)
        got = run(ext, monkeypatch, cs, True)
    finally:
        ext.set_deterministic(False)
    for name in ("dyeff1", "loss") + SUMS:
        assert torch.equal(got[name], want[name]), name
