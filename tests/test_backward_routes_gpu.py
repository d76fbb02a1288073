"""Each backward route is decided in one place, so its two entry points must
agree: the composite ops of the autograd path (conv_pool_bwd, linear_act_bwd)
against the fine-grained ops the fused step schedules one by one, and the
single-call form of FusedLeNetStep against its two-stage form.

Every shape here is one an existing GPU test already sends through one of
the two entry points (test_ops_gpu.py, test_conv2_dw_slab_gpu.py,
test_pool2_bwd_fused_gpu.py); nothing new reaches a kernel.  dX has no
atomics on any of these routes and is compared bitwise; dW / db accumulate
through fp32 atomics unless the route is single-writer, so each entry point is
held to the CPU reference with the tolerance of test_ops_gpu.py.
"""

import pytest
import torch

from test_ops_gpu import assert_close_bf16, to_gpu_bf16

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
    # the list test_pool2_bwd_fused_gpu.py clears
    for k in ("DMNIST_DW2_SLAB", "DMNIST_DW2_G", "DMNIST_DW2_KHB",
              "DMNIST_DW2_NBUF", "DMNIST_DW_G", "DMNIST_DW_SPREAD",
              "DMNIST_UNPOOL_LINES", "DMNIST_UNPOOL_TILE", "DMNIST_DX_PAIR",
              "DMNIST_DX_HIOCC", "DMNIST_DX_DB2SLIM", "DMNIST_POOL2_FUSED",
              "DMNIST_OVERLAP", "DMNIST_TWO_STREAM", "DMNIST_SINGLE_STREAM"):
        monkeypatch.delenv(k, raising=False)


def close(tag, got, ref):
    print(f"{tag}: max err={float((got.float().cpu() - ref).abs().max()):.3e} "
          f"(scale {float(ref.abs().max()):.3e})")
    assert_close_bf16(got, ref, scale=float(ref.abs().max()))


# ---------------------------------------------------------------------------
# conv: conv_pool_bwd against pool_scatter -> conv_dw_into -> conv_dx
# ---------------------------------------------------------------------------
_CONV = {}


def conv_case(ext, shape):
    """GPU inputs, the kernel's own (y, amax) and the CPU reference fed that
    routing, once per shape."""
    if shape not in _CONV:
        NB, H, W, Cin, Cout = shape
        torch.manual_seed(4)
        x = (torch.rand(NB, H, W, Cin) - 0.5).to(bf16).float()
        w = (torch.randn(5, 5, Cin, Cout) * 0.1).to(bf16).float()
        b = torch.randn(Cout) * 0.1
        dy = (torch.randn(NB, H // 2, W // 2, Cout) * 0.1).to(bf16).float()
        xg, wg, dyg = to_gpu_bf16(x), to_gpu_bf16(w), to_gpu_bf16(dy)
        yg, amaxg = ext.conv_pool_fwd(xg, wg, b.cuda().float())
        from distributedmnist_amd.ops import cpu_ref
        ref = cpu_ref.conv_pool_bwd(dy, x, w, yg.cpu().float(), amaxg.cpu())
        _CONV[shape] = (xg, wg, dyg, yg, amaxg, ref)
    return _CONV[shape]


def conv_both_entries(ext, shape):
    NB, H, W, Cin, Cout = shape
    need_dx = Cin > 1                      # conv1 is the first layer: no dx
    xg, wg, dyg, yg, amaxg, (dx_ref, dw_ref, db_ref) = conv_case(ext, shape)

    dx_c, dw_c, db_c = ext.conv_pool_bwd(dyg, xg, wg, yg, amaxg, need_dx)

    dw_p = torch.zeros(5, 5, Cin, Cout, device="cuda")
    db_p = torch.zeros(Cout, device="cuda")
    dact = ext.pool_scatter(dyg, yg, amaxg, db_p, H, W)
    ext.conv_dw_into(xg, dact, dw_p)
    if need_dx:
        dx_p = ext.conv_dx(dact, wg, Cin)
        assert torch.equal(dx_c, dx_p), "conv dX differs between the entries"
        close("dx", dx_c, dx_ref)
    else:
        assert dx_c.numel() == 0
    close("dw composite", dw_c, dw_ref)
    close("dw pieces", dw_p, dw_ref)
    close("db composite", db_c, db_ref)
    close("db pieces", db_p, db_ref)
    assert bool((dw_ref != 0).any()) and bool((db_ref != 0).any())


CONV2 = (8, 14, 14, 32, 64)


@pytest.mark.parametrize("shape", [CONV2, (3, 14, 14, 32, 64),
                                   (8, 28, 28, 1, 32)])
def test_conv_composite_matches_pieces(ext, shape):
    conv_both_entries(ext, shape)


@pytest.mark.parametrize("var,val", [("DMNIST_DW2_SLAB", "0"),   # conv_dw_tr
                                     ("DMNIST_DW_G", "4")])      # conv_dw_slab
def test_conv_composite_matches_pieces_routes(ext, monkeypatch, var, val):
    monkeypatch.setenv(var, val)           # both are read per call
    conv_both_entries(ext, CONV2)


# ---------------------------------------------------------------------------
# linear: linear_act_bwd against mask_db -> linear_dw_into -> linear_dx
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,N,relu", [(128, 3136, 512, True),
                                        (128, 512, 10, False)])
def test_linear_composite_matches_pieces(ext, B, K, N, relu):
    torch.manual_seed(2)
    x = (torch.randn(B, K) * 0.5).to(bf16).float()
    w = (torch.randn(K, N) * 0.1).to(bf16).float()
    b = torch.randn(N) * 0.1
    dy = (torch.randn(B, N) * 0.1).to(bf16).float()
    from distributedmnist_amd.ops import cpu_ref
    y = cpu_ref.linear_fwd(x, w, b, relu)
    dx_ref, dw_ref, db_ref = cpu_ref.linear_bwd(dy, x, w, y, relu)
    xg, wg, dyg, yg = (to_gpu_bf16(t) for t in (x, w, dy, y))

    dx_c, dw_c, db_c = ext.linear_act_bwd(dyg, xg, wg, yg, relu, 1.0, True)

    dw_p = torch.zeros(K, N, device="cuda")
    db_p = torch.zeros(N, device="cuda")
    dyeff = ext.mask_db(dyg, yg, relu, 1.0, db_p)
    ext.linear_dw_into(xg, dyeff, dw_p)
    dx_p = ext.linear_dx(dyeff, wg)

    assert torch.equal(dx_c, dx_p), "linear dX differs between the entries"
    close("dx", dx_c, dx_ref)
    if (B, K, N) == (128, 3136, 512):
        # split 1 into a fresh (16 B aligned) buffer: single writer, no atomics
        assert ext.linear_dw_plan(K, N, B)[2] == 1
        assert dw_p.data_ptr() % 16 == 0 and dw_c.data_ptr() % 16 == 0
        assert torch.equal(dw_c, dw_p), "single-writer dW differs"
    close("dw composite", dw_c, dw_ref)
    close("dw pieces", dw_p, dw_ref)
    close("db composite", db_c, db_ref)
    close("db pieces", db_p, db_ref)


# ---------------------------------------------------------------------------
# fused step: __call__ against stage_fc + stage_conv
# ---------------------------------------------------------------------------
def test_step_forms_agree(ext):
    """Eager, one GPU, no collectives, overlap level 0, B=64 (the batch of
    test_pool2_bwd_fused_gpu.py's step tests): both forms enqueue the same
    ops, so loss and accuracy (ordered softmax reduction) and the
    single-writer fc1_w gradient are bitwise equal; the gradients that
    accumulate through fp32 atomics agree within the eager-against-eager
    bound of test_ops_gpu.py::test_graphed_step_matches_eager."""
    from distributedmnist_amd.engine.fused_step import FusedLeNetStep
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    B = 64
    flags = build_train_parser().parse_args(
        ["--synthetic_data", "--train_dir", "/tmp/dm_routes_step",
         "--batch_size", str(B), "--max_steps", "1", "--model", "lenet",
         "--save_interval_secs", "100000", "--hip_graph", "off"])
    t = Trainer(flags, device=torch.device("cuda:0"))
    ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
    x, y = ds.next_batch(B)
    step = FusedLeNetStep(t)
    step.overlap_allreduce = False
    assert step.overlap_level == 0
    step_dev = torch.zeros(1, dtype=torch.int64, device=t.device)
    fp = t.fp

    def grads():
        torch.cuda.synchronize()
        return {n: fp.flat_grad[o:o + k].clone()
                for n, o, k in zip(fp.names, fp.offsets, fp.numels)}

    fp.flat_grad.zero_()
    loss1, acc1 = step(x, y, step_dev)
    g1, loss1, acc1 = grads(), loss1.clone(), acc1.clone()

    fp.flat_grad.zero_()
    loss2, acc2 = step.stage_fc(x, y, step_dev)
    step.stage_conv()
    g2 = grads()

    assert torch.equal(loss1, loss2) and torch.equal(acc1, acc2)
    assert ext.linear_dw_plan(3136, 512, B)[2] == 1
    assert torch.equal(g1["fc1_w"], g2["fc1_w"])
    # 0.02 is that test's constant; run-to-run atomic noise here is ~5e-7, so
    # this bound only catches a missing or doubled op.  The bitwise checks
    # above and the nonzero check carry the test.
    for name in fp.names:
        diff = float((g1[name] - g2[name]).abs().max())
        print(f"{name}: call-vs-stages {diff:.3e}")
        assert diff < 0.02, (name, diff)
        assert bool((g1[name] != 0).any()), name
