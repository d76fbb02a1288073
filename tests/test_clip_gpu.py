"""Global-norm gradient clipping on the GPU (--clip_grad_norm):
grad_norm_kernel against a float64 reference, the clipped sgd_step
instantiations against the CPU reference, and deterministic trainer runs,
graphed and eager."""

import math

import numpy as np
import pytest
import torch

from distributedmnist_amd.ops import cpu_ref
from distributedmnist_amd.ops import functional as Fx

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
CHUNK = 4096          # elements per block (csrc/kernels.h GRAD_NORM_CHUNK)
LENET_N = 1_663_370
LENET_NUMELS = [800, 32, 51200, 64, 1605632, 512, 5120, 10]
CANARY = 8


@pytest.fixture(scope="module")
def ext():
    from distributedmnist_amd import _C
    m = _C.ext()
    assert m is not None, "HIP extension must be present on GPU boxes"
    return m


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# -- grad_norm ----------------------------------------------------------------------

def one_segment(n):
    return [0], [n]


def lenet_table(n):
    assert n == LENET_N == sum(LENET_NUMELS)
    offs = np.concatenate([[0], np.cumsum(LENET_NUMELS)[:-1]])
    return [int(o) for o in offs], list(LENET_NUMELS)


def adversarial(n):
    """Odd offsets, a 1-element segment, a 2-element one, a 10-element
    segment across the first chunk boundary (4091..4101), a cut one past the
    third boundary, a 2-element tail: whatever of it fits into [0, n)."""
    cuts = sorted({c for c in (1, 3, 7, 1000, CHUNK - 5, CHUNK + 5,
                               2 * CHUNK + 3, 3 * CHUNK + 1, n - 3, n - 1)
                   if 0 < c < n})
    edges = [0] + cuts + [n]
    return edges[:-1], [b - a for a, b in zip(edges[:-1], edges[1:])]


TABLES = {"one": one_segment, "lenet": lenet_table, "odd": adversarial}
# 1, 3: a scalar tail alone; 4: one 16 B group; 1023: groups + tail in one
# block; a chunk - 1 / a chunk / + 1: the second block appears; 257 chunks + 5:
# the last block's threads take two partials each; the LeNet bucket
SIZES = [1, 3, 4, 1023, CHUNK - 1, CHUNK, CHUNK + 1, 257 * CHUNK + 5, LENET_N]
CASES = ([(n, "one") for n in SIZES] + [(LENET_N, "lenet")]
         + [(n, "odd") for n in SIZES if n >= 3])

_case = {}


def case(n, table):
    """(flat CPU fp32, offsets, numels), built once: randn scaled per segment
    over 1e-3 ... 1e3."""
    if (n, table) not in _case:
        offs, lens = TABLES[table](n)
        assert 1 <= len(offs) <= 16 and sum(lens) == n
        g = torch.Generator().manual_seed(1000 + n + len(offs))
        flat = torch.randn(n, generator=g)
        scales = (10.0 ** np.linspace(-3, 3, len(offs)) if len(offs) > 1
                  else [10.0])
        for o, m, s in zip(offs, lens, scales):
            flat[o:o + m] *= float(s)
        _case[(n, table)] = (flat, offs, lens)
    return _case[(n, table)]


def ref64(flat, offs, lens, scale):
    """[global, per segment ...] in python floats (float64 sums of the fp32
    values; the total is the sum of the segment sums)."""
    g = flat.double()
    sq = [float((g[o:o + m] ** 2).sum()) for o, m in zip(offs, lens)]
    return [scale * math.sqrt(sum(sq))] + [scale * math.sqrt(v) for v in sq]


def coef_of(norm, clip):
    """The kernel's formula in fp32, from the kernel's own norm."""
    f32 = np.float32
    return np.minimum(f32(1), f32(clip) / (f32(norm) + f32(1e-6)))


def launch(ext, g, offs, lens, scale, clip, steps=None):
    ns = len(offs)
    buf = torch.full((2 + ns + CANARY,), -7.5, device="cuda")
    if steps is None:
        steps = torch.zeros(1, dtype=torch.int64, device="cuda")
    ext.grad_norm(g, offs, lens, scale, clip, buf[:2 + ns], steps)
    return buf, steps


def check_stats(ext, flat, offs, lens, scale, tag):
    n, ns = flat.numel(), len(offs)
    blocks, chain = ext.grad_norm_plan(n)
    assert blocks == -(-n // CHUNK) and 1 <= chain
    want = ref64(flat, offs, lens, scale)
    # ops/cpu_ref.py::grad_norm is this reference rounded to fp32
    cref = cpu_ref.grad_norm(flat, offs, lens, scale, math.inf)
    for a, b in zip(cref[[0] + list(range(2, 2 + ns))].tolist(), want):
        assert abs(a - b) <= EPS * b
    g = flat.cuda()
    before = bits(g)
    buf, steps = launch(ext, g, offs, lens, scale, math.inf)
    got = buf[:2 + ns].cpu()
    assert float(got[1]) == 1.0 and int(steps) == 0  # inf never clips
    worst = 0.0
    for i, w in zip([0] + list(range(2, 2 + ns)), want):
        err = abs(float(got[i]) - w)
        assert err <= (chain + 4) * EPS * w, (tag, i, float(got[i]), w)
        worst = max(worst, err / (EPS * w) if w else 0.0)
    print(f"{tag}: blocks {blocks} chain {chain}, worst norm error "
          f"{worst:.2f} x 2^-24 (bound {chain + 4})")
    norm = float(got[0])
    assert norm > 0
    for clip, clipped in ((norm / 2, 1), (norm * 2, 0), (0.75 * norm, 1)):
        b2, steps = launch(ext, g, offs, lens, scale, clip, steps)
        # the same launch twice: the same bits
        b3, s3 = launch(ext, g, offs, lens, scale, clip)
        assert torch.equal(bits(b2), bits(b3)) and int(s3) == clipped
        assert torch.equal(bits(b2[2:]), bits(buf[2:]))
        assert float(b2[0]) == norm
        c = coef_of(norm, clip)
        assert abs(float(b2[1]) - float(c)) <= 4 * float(np.spacing(c))
        assert (float(b2[1]) < 1.0) == bool(clipped)
    assert int(steps) == 2  # + 1, + 0, + 1
    assert bool((buf[2 + ns:] == -7.5).all())  # canaries past stats
    assert bool((b2[2 + ns:] == -7.5).all())
    assert torch.equal(bits(g), before)        # grad is read only


@pytest.mark.parametrize("n,table", CASES)
def test_grad_norm_against_float64(ext, n, table):
    flat, offs, lens = case(n, table)
    scale = 1.0 / 3 if table == "lenet" else (0.5 if n % 2 else 1.0)
    check_stats(ext, flat, offs, lens, scale, f"n={n} {table}")


def test_chain_at_the_lenet_size_is_short(ext):
    blocks, chain = ext.grad_norm_plan(LENET_N)
    assert chain <= 64 and 256 <= blocks <= 1024
    # larger buckets: longer chunks, never more blocks than the workspace
    for n in (1, CHUNK * 1024, CHUNK * 1024 + 1, 1 << 33):
        b, c = ext.grad_norm_plan(n)
        assert 1 <= b <= 1024 and c >= chain - 2
    with pytest.raises(RuntimeError):
        ext.grad_norm_plan(0)


@pytest.mark.parametrize("table", ["one", "lenet", "odd"])
def test_grad_norm_zero_bucket_and_last_element(ext, table):
    offs, lens = TABLES[table](LENET_N)
    ns = len(offs)
    g = torch.zeros(LENET_N, device="cuda")
    buf, steps = launch(ext, g, offs, lens, 1.0, 0.5)
    got = buf[:2 + ns].cpu()
    assert not bool(torch.isnan(got).any())
    assert float(got[0]) == 0.0 and float(got[1]) == 1.0
    assert not bool(got[2:].any()) and int(steps) == 0
    g[-1] = -3.0
    buf, steps = launch(ext, g, offs, lens, 0.5, 0.5, steps)
    got = buf[:2 + ns].cpu()
    assert float(got[0]) == 1.5 and float(got[-1]) == 1.5
    assert not bool(got[2:-1].any())
    c = coef_of(1.5, 0.5)
    assert abs(float(got[1]) - float(c)) <= 4 * float(np.spacing(c))
    assert int(steps) == 1
    assert bool((buf[2 + ns:] == -7.5).all())


def test_grad_norm_repeats_under_a_busy_device(ext):
    """Every other launch runs beside two 2048^2 matrix products on a second
    stream (the perturbation of tests/test_deterministic_gpu.py)."""
    flat, offs, lens = case(LENET_N, "lenet")
    g = flat.cuda()
    a = torch.randn(2048, 2048, device="cuda")
    side = torch.cuda.Stream()
    outs = []
    for i in range(6):
        if i % 2:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                torch.mm(a, a)
                torch.mm(a, a)
        outs.append(launch(ext, g, offs, lens, 1.0, 1.0)[0].clone())
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(bits(o), bits(outs[0]))


def test_grad_norm_refuses_bad_arguments(ext):
    g = torch.zeros(16, device="cuda")
    st = torch.zeros(4, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ext.grad_norm(g, [0, 6], [6, 10], 1.0, 1.0, st, cnt)
    for offs, lens in (([0, 6], [6, 9]), ([0, 7], [6, 10]), ([1, 6], [5, 10])):
        with pytest.raises(RuntimeError, match="tile"):
            ext.grad_norm(g, offs, lens, 1.0, 1.0, st, cnt)
    with pytest.raises(RuntimeError, match="segments"):
        ext.grad_norm(g, list(range(16)) + [16], [1] * 16 + [0], 1.0, 1.0,
                      torch.zeros(19, device="cuda"), cnt)
    with pytest.raises(RuntimeError, match="stats"):
        ext.grad_norm(g, [0], [16], 1.0, 1.0, st, cnt)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match="clip"):
            ext.grad_norm(g, [0, 6], [6, 10], 1.0, bad, st, cnt)
    with pytest.raises(RuntimeError, match="aligned"):
        ext.grad_norm(torch.zeros(17, device="cuda")[1:], [0, 6], [6, 10],
                      1.0, 1.0, st, cnt)
    with pytest.raises(RuntimeError, match="int64"):
        ext.grad_norm(g, [0, 6], [6, 10], 1.0, 1.0, st, cnt.int())


def test_functional_grad_norm_dispatches(ext):
    flat, offs, lens = case(1023, "odd")
    want = cpu_ref.grad_norm(flat, offs, lens, 0.5, 2.0)
    assert torch.equal(Fx.grad_norm(flat, offs, lens, 0.5, 2.0), want)
    got = Fx.grad_norm(flat.cuda(), offs, lens, 0.5, 2.0)
    assert got.is_cuda and got.shape == want.shape
    _, chain = ext.grad_norm_plan(1023)
    assert float(((got.cpu() - want).abs()[2:]
                  / want[2:]).max()) <= (chain + 5) * EPS


# -- the clipped SGD instantiations ---------------------------------------------------

# powers of two (tests/test_ema_gpu.py): coef*g, lr*g and mu*v are exact, so
# the kernel's fused multiply-adds and the reference's separate multiply + add
# round the same values and the masters agree bit for bit
LR, MU, COEF, D = 0.125, 0.5, 0.25, 0.5
OFFSET0 = 6
PAD = 8


def ema_atol(n_updates, masters):
    """4 * n * 2^-24 * max|w| (tests/test_ema_cpu.py)."""
    return 4 * n_updates * EPS * max(float(w.abs().max()) for w in masters)


_sgd_in, _sgd_ref = {}, {}


def sgd_inputs(n):
    if n not in _sgd_in:
        g = torch.Generator().manual_seed(77 + n)
        _sgd_in[n] = (torch.randn(n, generator=g),
                      [torch.randn(n, generator=g) for _ in range(3)])
    return _sgd_in[n]


def sgd_reference(n, momentum, ema):
    """Three clipped updates through ops/cpu_ref.py, once per case:
    per-update (master, momentum, average, shadow)."""
    key = (n, momentum, ema)
    if key not in _sgd_ref:
        w0, grads = sgd_inputs(n)
        m = w0.clone()
        e = w0.clone() if ema else None
        v = torch.zeros(n) if momentum else None
        sh = torch.zeros(n, dtype=torch.bfloat16)
        out = []
        for i, g in enumerate(grads):
            cpu_ref.sgd_step(m, g, LR, shadow=sh, momentum=v,
                             mu=MU if momentum else 0.0, ema=e,
                             ema_decay=D if ema else 0.0,
                             offset=OFFSET0 + i,
                             clip_coef=torch.tensor([COEF]))
            out.append((m.clone(), None if v is None else v.clone(),
                        None if e is None else e.clone(), sh.clone()))
        _sgd_ref[key] = out
    return _sgd_ref[key]


@pytest.mark.parametrize("mode", ["value", "dev", "dev_zero"])
@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("momentum", [False, True], ids=["sgd", "momentum"])
@pytest.mark.parametrize("n", [1, 5, 1027])
def test_clipped_sgd_step_matches_cpu_reference(ext, n, momentum, ema, mode):
    w0, grads = sgd_inputs(n)
    ref = sgd_reference(n, momentum, ema)
    master = torch.full((n + PAD,), 7.5, device="cuda")
    master[:n] = w0.cuda()
    ebuf = master.clone() if ema else None
    mom = torch.zeros(n, device="cuda") if momentum else None
    shadow = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    # the coefficient sits where grad_norm leaves it: element 1 of the stats
    stats = torch.tensor([3.0, COEF, 9.0], device="cuda")
    lr_dev = torch.tensor([LR], device="cuda")
    mu = MU if momentum else 0.0
    kw = dict(momentum=mom, mu=mu, clip_coef=stats[1:2])
    if ema:
        kw.update(ema=ebuf[:n], ema_decay=D)
    for i, g in enumerate(grads):
        gg = g.cuda()
        if mode == "value":
            ext.sgd_step(master[:n], gg, shadow, True, LR, 1.0, -1.0, 0,
                         OFFSET0 + i, **kw)
            assert torch.equal(gg, g.cuda())
        else:
            off_dev = torch.tensor([OFFSET0 + i], dtype=torch.int64,
                                   device="cuda")
            ext.sgd_step_dev(master[:n], gg, shadow, True, lr_dev, -1.0, 0,
                             off_dev, zero_grad=(mode == "dev_zero"), **kw)
            if mode == "dev_zero":
                assert not bool(gg.any())
            else:
                assert torch.equal(gg, g.cuda())
        m_ref, v_ref, e_ref, sh_ref = ref[i]
        assert torch.equal(bits(master[:n]), bits(m_ref)), (n, i)
        assert torch.equal(shadow.cpu().view(torch.int16),
                           sh_ref.view(torch.int16))
        if momentum:
            assert torch.equal(bits(mom), bits(v_ref))
        if ema:
            err = float((ebuf[:n].cpu().double() - e_ref.double()).abs().max())
            assert err <= ema_atol(i + 1, [r[0] for r in ref[:i + 1]])
            assert bool((ebuf[n:] == 7.5).all())
        assert bool((master[n:] == 7.5).all())  # canaries
    assert stats.tolist() == [3.0, COEF, 9.0]
    # and the clip really changed the update
    plain = w0.clone()
    cpu_ref.sgd_step(plain, grads[0], LR)
    assert not torch.equal(plain, ref[0][0])


def test_sgd_step_without_a_coefficient_is_unchanged(ext):
    """clip_coef = a device 1.0 gives the bits of the call without it."""
    n = 1027
    w0, grads = sgd_inputs(n)
    one = torch.ones(1, device="cuda")
    out = []
    for kw in ({}, {"clip_coef": one}):
        m, v = w0.cuda(), torch.zeros(n, device="cuda")
        sh = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
        for i, g in enumerate(grads):
            ext.sgd_step(m, g.cuda(), sh, True, 0.1, 1.0, 0.9, 3, i,
                         momentum=v, mu=0.9, **kw)
        out.append((m, v))
    assert torch.equal(bits(out[0][0]), bits(out[1][0]))
    assert torch.equal(bits(out[0][1]), bits(out[1][1]))
    with pytest.raises(RuntimeError, match="clip_coef"):
        ext.sgd_step(out[0][0], grads[0].cuda(), sh, True, 0.1, 1.0, -1.0, 0,
                     0, clip_coef=torch.ones(2, device="cuda"))


# -- deterministic trainer runs ---------------------------------------------------------

B, STEPS = 192, 4
_runs = {}


def trainer_run(tmp_path_factory, graph, clip, again=0):
    """(masters after the last step, clip_stats, clipped_steps, grad_norms()
    after the first step), once per (graph, clip, again)."""
    key = (graph, clip, again)
    if key in _runs:
        return _runs[key]
    from distributedmnist_amd import _C
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    argv = ["--synthetic_data", "--model", "lenet", "--deterministic",
            "--batch_size", str(B), "--max_steps", str(STEPS),
            "--initial_learning_rate", "0.05", "--momentum", "0.9",
            "--save_interval_secs", "100000", "--train_dir",
            str(tmp_path_factory.mktemp("clipdet"))]
    if not graph:
        argv += ["--hip_graph", "off"]
    if clip is not None:
        argv += ["--clip_grad_norm", repr(clip)]
    flags = build_train_parser().parse_args(argv)
    try:
        t = Trainer(flags, device=torch.device("cuda:0"))
        ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
        first = None
        for i in range(STEPS):
            x, y = ds.next_batch(B)
            _, loss, _, _ = t.graph_or_eager_step(x, y)
            assert float(loss) == float(loss)
            if i == 0 and clip is not None:
                first = t.grad_norms()
        torch.cuda.synchronize()
        assert (t._graph is not None) == graph, "capture must engage"
        _runs[key] = (t.fp.flat_master.cpu(),
                      None if clip is None else t.clip_stats.cpu(),
                      None if clip is None else int(t.clipped_steps),
                      first, t.clip_updates)
    finally:
        _C.ext().set_deterministic(False)
    return _runs[key]


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_trainer_inf_is_the_flag_off_run(tmp_path_factory, graph):
    w_off, s_off, c_off, _, _ = trainer_run(tmp_path_factory, graph, None)
    w_inf, stats, clipped, first, updates = trainer_run(
        tmp_path_factory, graph, math.inf)
    assert s_off is None and c_off is None
    assert torch.equal(bits(w_inf), bits(w_off))
    assert clipped == 0 and updates == STEPS  # the warm-up left no trace
    assert float(stats[1]) == 1.0 and first["clip_coef"] == 1.0
    assert all(math.isfinite(v) and v > 0 for v in first.values())
    assert all(math.isfinite(v) and v > 0 for v in stats.tolist())


def test_trainer_clipped_runs_agree_bitwise(tmp_path_factory):
    _, _, _, first, _ = trainer_run(tmp_path_factory, True, math.inf)
    _, _, _, first_e, _ = trainer_run(tmp_path_factory, False, math.inf)
    assert first == first_e
    clip = first["global"] / 2
    g1 = trainer_run(tmp_path_factory, True, clip)
    g2 = trainer_run(tmp_path_factory, True, clip, again=1)
    e1 = trainer_run(tmp_path_factory, False, clip)
    w_inf = trainer_run(tmp_path_factory, True, math.inf)[0]
    print(f"first norm {first['global']!r}, clip {clip!r}, clipped steps "
          f"{g1[2]} of {g1[4]}, last stats {g1[1].tolist()[:2]}")
    for other in (g2, e1):
        assert torch.equal(bits(other[0]), bits(g1[0]))
        assert torch.equal(bits(other[1]), bits(g1[1]))
        assert other[2] == g1[2] and other[4] == g1[4] == STEPS
        assert other[3] == g1[3]
    assert g1[2] >= 1
    assert g1[3]["global"] == first["global"]
    assert abs(g1[3]["clip_coef"] - float(coef_of(first["global"], clip))) \
        <= 4 * float(np.spacing(np.float32(g1[3]["clip_coef"])))
    assert not torch.equal(bits(g1[0]), bits(w_inf))  # clipping changed it
