"""LARS on the GPU (--lars_eta): lars_norm_kernel against float64 and against
grad_norm_kernel's bits, the LARS instantiations of the SGD pass against the
CPU reference, and deterministic trainer runs, graphed and eager."""

import math

import numpy as np
import pytest
import torch
from test_clip_gpu import CHUNK, LENET_N, TABLES, bits
from test_clip_gpu import ext  # noqa: F401  (the extension fixture)

from distributedmnist_amd.ops import cpu_ref

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
ETA = float(np.float32(0.001))
f32 = np.float32


# -- lars_norm ------------------------------------------------------------------------

# n = 5 / 1027 / two chunks + 77 on the odd table (odd offsets, a 1-element
# tensor, 10 elements across the first chunk boundary), the LeNet bucket
CASES = [(1, "one"), (5, "odd"), (1027, "odd"), (2 * CHUNK + 77, "odd"),
         (LENET_N, "lenet")]
_case = {}


def case(n, table):
    """(master, grad, offsets, numels, float64 sum w^2, sum g^2), once."""
    if (n, table) not in _case:
        offs, lens = TABLES[table](n)
        g = torch.Generator().manual_seed(31 + n)
        w, gr = torch.randn(n, generator=g), 3 * torch.randn(n, generator=g)
        sq = [[float((x.double()[o:o + m] ** 2).sum())
               for o, m in zip(offs, lens)] for x in (w, gr)]
        _case[(n, table)] = (w, gr, offs, lens, sq[0], sq[1])
    return _case[(n, table)]


def run_lars(ext, w, g, offs, lens, adapt, scale, wd, clip):
    ns = len(offs)
    tab = torch.full((32,), -7.5, device="cuda")
    st = torch.full((3 * ns,), -7.5, device="cuda")
    cs = torch.full((2 + ns,), -7.5, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ext.lars_norm(w, g, offs, lens, adapt, scale, ETA, wd, clip, tab, st,
                  clip_stats=cs, clipped_steps=cnt)
    return tab.cpu(), st.cpu(), cs.cpu(), int(cnt)


@pytest.mark.parametrize("clipped", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("n,table", CASES)
def test_lars_norm_against_float64(ext, n, table, clipped):
    """wn, gn within E = (chain + 4) * 2^-24, ratio within (2E + 8) * 2^-24 of
    float64 (docs/KERNELS.md "LARS").  With a clip that bites the float64
    coefficient is the reference too and the kernel's own (norm E, + 1e-6,
    quotient: E + 2, one of slack) is added to the bounds of gn and ratio."""
    w, g, offs, lens, sw, sg = case(n, table)
    ns = len(offs)
    blocks, chain = ext.lars_norm_plan(n)
    assert (blocks, chain) == tuple(ext.grad_norm_plan(n))
    E = chain + 4
    extra = E + 3 if clipped else 0
    adapt = 0x5555 & ((1 << ns) - 1) if ns > 1 else 1
    wc, gc = w.cuda(), g.cuda()
    worst = [0.0, 0.0, 0.0]
    for scale in (1.0, 1.0 / 3):
        s32 = float(f32(scale))
        norm = s32 * math.sqrt(sum(sg))
        clip = float(f32(norm / 2)) if clipped else 0.0
        coef = clip / (norm + 1e-6) if clipped else 1.0
        for wd in (0.0, float(f32(5e-4))):
            tab, st, cs, cnt = run_lars(ext, wc, gc, offs, lens, adapt, scale,
                                        wd, clip)
            again = run_lars(ext, wc, gc, offs, lens, adapt, scale, wd, clip)
            assert all(torch.equal(bits(a), bits(b))
                       for a, b in zip((tab, st, cs), again[:3]))
            if clipped:  # the g side is grad_norm_kernel's, bit for bit
                ref = torch.empty(2 + ns, device="cuda")
                rcnt = torch.zeros(1, dtype=torch.int64, device="cuda")
                ext.grad_norm(gc, offs, lens, scale, clip, ref, rcnt)
                assert torch.equal(bits(cs), bits(ref))
                assert cnt == int(rcnt) == 1
            else:
                assert bool((cs == -7.5).all()) and cnt == 0
            kcoef = float(cs[1]) if clipped else 1.0
            assert bool((tab[2 * ns:] == -7.5).all())
            for t in range(ns):
                wn, gn = math.sqrt(sw[t]), coef * s32 * math.sqrt(sg[t])
                kwn, kgn, kr = (float(v) for v in st[3 * t:3 * t + 3])
                errs = [abs(kwn - wn) / wn / EPS, abs(kgn - gn) / gn / EPS]
                assert errs[0] <= E and errs[1] <= E + extra, (t, errs)
                if (adapt >> t) & 1:
                    ratio = ETA * wn / (gn + wd * wn)
                    errs.append(abs(kr - ratio) / ratio / EPS)
                    assert errs[2] <= 2 * E + 8 + extra, (t, errs)
                    d = kr * wd / s32
                    assert abs(float(tab[2 * t + 1]) - d) <= 2 * EPS * d
                else:  # left alone: a_t = coef, d_t = 0, exactly
                    assert kr == 1.0 and float(tab[2 * t]) == kcoef
                    assert float(tab[2 * t + 1]) == 0.0
                a = kr * kcoef
                assert abs(float(tab[2 * t]) - a) <= 2 * EPS * a
                worst = [max(p, q) for p, q in zip(worst, errs + [0.0])]
    print(f"n={n} {table} {'clip' if clipped else 'noclip'}: chain {chain}, "
          f"worst wn {worst[0]:.2f} gn {worst[1]:.2f} ratio {worst[2]:.2f} "
          f"x 2^-24 (bounds {E}, {E + extra}, {2 * E + 8 + extra})")


@pytest.mark.parametrize("zero", ["grad", "master"])
def test_a_zero_tensor_has_ratio_one(ext, zero):
    w, g, offs, lens, _, _ = case(1027, "odd")
    w, g = w.clone(), g.clone()
    (g if zero == "grad" else w)[offs[3]:offs[3] + lens[3]] = 0.0
    tab, st, _, _ = run_lars(ext, w.cuda(), g.cuda(), offs, lens, 0xFFFF
                             & ((1 << len(offs)) - 1), 1.0, 5e-4, 0.0)
    assert not bool(torch.isnan(st).any())
    assert float(st[3 * 3 + 2]) == 1.0 and float(tab[2 * 3]) == 1.0
    assert float(st[3 * 2 + 2]) != 1.0
    with pytest.raises(RuntimeError, match="eta"):
        ext.lars_norm(w.cuda(), g.cuda(), offs, lens, 1, 1.0, 0.0, 0.0, 0.0,
                      tab.cuda(), st.cuda())


# -- the LARS instantiations of the SGD pass ------------------------------------------

# powers of two throughout (tests/test_clip_gpu.py): a*g, d*w, mu*v and lr*v
# are exact, so contracting a*g + d*w or not rounds the same value
LR, MU, D, OFFSET0, PAD = 0.125, 0.5, 0.5, 6, 8
# a boundary inside a 16 B group: 3 of 0..3; 6 of 4..7 (with an empty tensor
# there) and 1001 of 1000..1003
SGD_TABLES = {1: ([0], [1]), 5: ([0, 3], [3, 2]),
              1027: ([0, 6, 6, 1001], [6, 0, 995, 26])}
PAIRS = [0.5, 0.25, 2.0, 0.0, 1.0, 0.5, 0.25, 0.125] + [64.0] * 24
_sgd_ref = {}


def sgd_reference(n, momentum, ema):
    """Three LARS updates through ops/cpu_ref.py, once per case."""
    key = (n, momentum, ema)
    if key not in _sgd_ref:
        g = torch.Generator().manual_seed(77 + n)
        w0 = torch.randn(n, generator=g)
        grads = [torch.randn(n, generator=g) for _ in range(3)]
        m, e = w0.clone(), (w0.clone() if ema else None)
        v = torch.zeros(n) if momentum else None
        sh = torch.zeros(n, dtype=torch.bfloat16)
        offs, lens = SGD_TABLES[n]
        out = []
        for i, gr in enumerate(grads):
            cpu_ref.sgd_step(m, gr, LR, shadow=sh, momentum=v,
                             mu=MU if momentum else 0.0, ema=e,
                             ema_decay=D if ema else 0.0, offset=OFFSET0 + i,
                             lars_tab=torch.tensor(PAIRS), offsets=offs,
                             numels=lens)
            out.append((m.clone(), None if v is None else v.clone(),
                        None if e is None else e.clone(), sh.clone()))
        _sgd_ref[key] = (w0, grads, out)
    return _sgd_ref[key]


@pytest.mark.parametrize("mode", ["value", "dev", "dev_zero"])
@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("momentum", [False, True], ids=["sgd", "momentum"])
@pytest.mark.parametrize("n", [1, 5, 1027])
def test_lars_sgd_step_matches_cpu_reference(ext, n, momentum, ema, mode):
    w0, grads, ref = sgd_reference(n, momentum, ema)
    offs, lens = SGD_TABLES[n]
    master = torch.full((n + PAD,), 7.5, device="cuda")
    master[:n] = w0.cuda()
    ebuf = master.clone() if ema else None
    mom = torch.zeros(n, device="cuda") if momentum else None
    shadow = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    lr_dev = torch.tensor([LR], device="cuda")
    kw = dict(momentum=mom, mu=MU if momentum else 0.0,
              lars_tab=torch.tensor(PAIRS, device="cuda"), offsets=offs,
              numels=lens)
    if ema:
        kw.update(ema=ebuf[:n], ema_decay=D)
    for i, g in enumerate(grads):
        gg = g.cuda()
        if mode == "value":
            ext.sgd_step(master[:n], gg, shadow, True, LR, 1.0, -1.0, 0,
                         OFFSET0 + i, **kw)
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
        if ema:  # 4 * updates * 2^-24 * max|w| (tests/test_ema_cpu.py)
            err = float((ebuf[:n].cpu().double() - e_ref.double()).abs().max())
            assert err <= 4 * (i + 1) * EPS * max(
                float(r[0].abs().max()) for r in ref[:i + 1])
            assert bool((ebuf[n:] == 7.5).all())
        assert bool((master[n:] == 7.5).all())  # canaries


def test_an_identity_table_is_the_call_without_one(ext):
    """Masked and with momentum; lars_tab with clip_coef is refused."""
    n = 1027
    w0, grads, _ = sgd_reference(n, True, False)
    offs, lens = SGD_TABLES[n]
    ident = torch.tensor([1.0, 0.0] * 16, device="cuda")
    out = []
    for kw in ({}, dict(lars_tab=ident, offsets=offs, numels=lens)):
        m, v = w0.cuda(), torch.zeros(n, device="cuda")
        sh = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
        for i, g in enumerate(grads):
            ext.sgd_step(m, g.cuda(), sh, True, 0.1, 1.0, 0.9, 3, i,
                         momentum=v, mu=0.9, **kw)
        out.append((m, v))
    assert torch.equal(bits(out[0][0]), bits(out[1][0]))
    assert torch.equal(bits(out[0][1]), bits(out[1][1]))
    with pytest.raises(RuntimeError, match="mutually exclusive"):
        ext.sgd_step(m, grads[0].cuda(), sh, True, 0.1, 1.0, -1.0, 0, 0,
                     clip_coef=ident[:1], lars_tab=ident, offsets=offs,
                     numels=lens)


# -- deterministic trainer runs ---------------------------------------------------------

B, STEPS = 64, 3


def trainer_run(tmp_path, tag, graph, clip):
    from distributedmnist_amd import _C
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    argv = ["--synthetic_data", "--model", "lenet", "--deterministic",
            "--batch_size", str(B), "--max_steps", str(STEPS),
            "--lars_eta", "0.001", "--weight_decay", "5e-4", "--momentum",
            "0.9", "--save_interval_secs", "100000", "--train_dir",
            str(tmp_path / tag)]
    argv += [] if graph else ["--hip_graph", "off"]
    argv += ["--clip_grad_norm", "1"] if clip else []
    flags = build_train_parser().parse_args(argv)
    try:
        t = Trainer(flags, device=torch.device("cuda:0"))
        ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
        for _ in range(STEPS):
            x, y = ds.next_batch(B)
            _, loss, _, _ = t.graph_or_eager_step(x, y)
            assert float(loss) == float(loss)
        torch.cuda.synchronize()
        assert (t._graph is not None) == graph, "capture must engage"
        return (t.fp.flat_master.cpu(), t.trust_ratios(),
                t.grad_norms() if clip else None)
    finally:
        _C.ext().set_deterministic(False)


@pytest.mark.parametrize("clip", [False, True], ids=["lars", "lars_clip"])
def test_trainer_runs_agree_bitwise(tmp_path, clip):
    g1 = trainer_run(tmp_path, "g1", True, clip)
    e1 = trainer_run(tmp_path, "e1", False, clip)
    g2 = trainer_run(tmp_path, "g2", True, clip)
    for other in (e1, g2):
        assert torch.equal(bits(other[0]), bits(g1[0]))
        assert other[1] == g1[1] and other[2] == g1[2]
    ratios = g1[1]
    assert all(math.isfinite(v) and v >= 0 for r in ratios.values() for v in r)
    assert all((r[2] == 1.0) == name.endswith("_b")
               for name, r in ratios.items()), ratios
    if clip:
        assert g1[2]["global"] > 0 and 0 < g1[2]["clip_coef"] <= 1.0
