"""--optimizer adam|lamb on the GPU: adam_step_kernel, lamb_moments_kernel and
lamb_apply_kernel against a float64 replay and ops/cpu_ref.py, LAMB's
reproducibility, and trainer runs, eager and graphed.

The bound of the float64 comparison, per update, from the fp32 values the
update starts from (e = 2^-24, every kernel operation one rounding; derived
step by step in docs/KERNELS.md "Adam and LAMB", computed by replay()):
  m': Em = e(|b1 m| + 3|(1-b1) gh| + |m'|)      v': 7e v'
  u_t: Eut = 8e|u| + (Em + 3e|m'|)/(c1 den) + e|wd w| + e|u_t|
  adam w': lr Eut + e|lr u_t| + e|w'|
  lamb |w_t|, |u_t|: (chain + 4)e (lamb_norm_plan), |u_t| also |Eut|_2/|u_t|;
       r: Er = (2(chain + 4) + 1)e + |Eut|_2/|u_t|
       w': |lr r u_t|(Er + 2e) + lr r Eut + e|w'|
all times 1.001 for the second-order terms."""

import functools
import math

import numpy as np
import pytest
import torch
from test_clip_gpu import bits
from test_clip_gpu import ext  # noqa: F401  (the extension fixture)

from distributedmnist_amd.ops import cpu_ref
from distributedmnist_amd.ops import functional as Fx

pytestmark = pytest.mark.gpu

EPS, SLACK = 2.0 ** -24, 1.001
f32 = np.float32
LR, B1, B2, AEPS, WD, D, SEED, KEEP, PAD = 0.01, 0.9, 0.999, 1e-8, 0.01, 0.5, 3, 0.75, 8
# straddled groups, a whole chunk, one element, a chunk boundary + scalar tail
SMALL = (5, 3, 4096, 1, 4100)
# blocks take more than one chunk (GRAD_NORM_MAX_BLOCKS * GRAD_NORM_CHUNK)
BIG = (5, 3, 1024 * 4096 + 4099 - 8)
ADAPT = 0b11101


@functools.lru_cache(None)
def layout(lens):
    """(offsets, numels, adapt, w0, three gradients: the sum over 2
    contributors), once per segment layout."""
    g = torch.Generator().manual_seed(len(lens))
    n = sum(lens)
    return ([sum(lens[:i]) for i in range(len(lens))], list(lens),
            ADAPT & ((1 << len(lens)) - 1), torch.randn(n, generator=g),
            [2 * torch.randn(n, generator=g) for _ in range(3)])


def replay(opt, w, g, m, v, k, s, coef, mask, lr, offs, lens, adapt, chain):
    """One update in float64 -> (w', m', v', stats, bound on w', on m')."""
    b1, b2, o1, o2 = (float(f32(x)) for x in (B1, B2, 1 - B1, 1 - B2))
    c1, c2 = (-math.expm1(k * float(f32(math.log(b)))) for b in (B1, B2))
    gh = coef * s * g * mask
    a, b = b1 * m, o1 * gh
    m2, v2 = a + b, b2 * v + o2 * gh * gh
    den = (v2 / c2).sqrt() + float(f32(AEPS))
    u = m2 / c1 / den
    Em = EPS * (a.abs() + 3 * b.abs() + m2.abs())
    Eu = 8 * EPS * u.abs() + (Em + 3 * EPS * m2.abs()) / (c1 * den)
    w2, Ew, stats = w.clone(), torch.zeros_like(w), []
    for t, (o, n) in enumerate(zip(offs, lens)):
        sl = slice(o, o + n)
        ad = bool((adapt >> t) & 1)
        dec = (float(f32(WD)) if ad else 0.0) * w[sl]
        ut = u[sl] + dec
        Eut = Eu[sl] + EPS * dec.abs() + EPS * ut.abs()
        r, Er = 1.0, 0.0
        if opt == "lamb":
            wn, un = float(w[sl].norm()), float(ut.norm())
            En = (chain + 4) * EPS
            if ad and wn > 0 and un > 0:
                r = wn / un
                Er = (2 * (chain + 4) + 1) * EPS + float(Eut.norm()) / un
            stats.append((wn, un, r, En, En + float(Eut.norm()) / max(un, 1e-300), Er))
        p = lr * r * ut
        w2[sl] = w[sl] - p
        Ew[sl] = (p.abs() * (Er + 2 * EPS) + lr * r * Eut + EPS * w2[sl].abs())
    return w2, m2, v2, stats, SLACK * Ew, SLACK * Em


# ema x clip, and one --drop_connect_post case through the *_dev launchers
CASES = [(False, False, False), (True, False, False), (False, True, False),
         (True, True, False), (False, False, True)]
PARAMS = [(o, SMALL, *c) for o in ("adam", "lamb") for c in CASES] + [
    ("lamb", BIG, False, False, False), ("lamb", BIG, True, True, False)]


@pytest.mark.parametrize("opt,lens,ema,clip,dc", PARAMS, ids=[
    f"{p[0]}-{len(p[1])}" + "-ema" * p[2] + "-clip" * p[3] + "-dc_dev" * p[4]
    for p in PARAMS])
def test_update_against_float64_and_cpu_ref(ext, opt, lens, ema, clip, dc):
    offs, lens, adapt, w0, grads = layout(lens)
    n = w0.numel()
    _, chain = ext.lamb_norm_plan(n)
    buf = {name: torch.full((n + PAD,), 7.5, device="cuda")
           for name in "wmveg"}
    w, m, v, e, gbuf = (buf[c][:n] for c in "wmveg")
    w.copy_(w0); e.copy_(w0); m.zero_(); v.zero_()
    sh = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    coef = torch.tensor([0.625], device="cuda") if clip else None
    tab, st = torch.ones(16, device="cuda"), torch.zeros(3 * len(offs), device="cuda")
    hp = dict(beta1=B1, beta2=B2, eps=AEPS, wd=WD, offsets=offs, numels=lens,
              adapt_mask=adapt)
    # the CPU reference runs its own chain from the same start
    rw, rm, rv, re = w0.clone(), torch.zeros(n), torch.zeros(n), w0.clone()
    worst = 0.0
    for i, g in enumerate(grads):
        mask = torch.ones(n)
        if dc:  # the SGD pass's own mask: w = 0 - 1 * (1 * mask)
            z = torch.zeros(n, device="cuda")
            ext.sgd_step(z, torch.ones(n, device="cuda"), z, False, 1.0, 1.0,
                         KEEP, SEED, i)
            mask = (z != 0).float().cpu()
        gbuf.copy_(g)
        before = [x.cpu().double() for x in (w, m, v)]
        e_before = e.cpu()
        kw = dict(hp, drop_connect_keep=KEEP if dc else None, seed=SEED,
                  offset=i, shadow=sh, ema=e if ema else None,
                  ema_decay=D if ema else 0.0, clip_coef=coef)
        if dc:
            kw.update(lr_scale_dev=torch.tensor([LR * 0.5], device="cuda"),
                      offset_dev=torch.tensor([i], device="cuda"),
                      zero_grad=True, offset=0)
        if opt == "adam":
            Fx.adam_step(w, gbuf, m, v, 0.0 if dc else LR, 0.5, **kw)
        else:
            Fx.lamb_step(w, gbuf, m, v, 0.0 if dc else LR, 0.5,
                         lamb_tab=tab, lamb_stats=st, **kw)
        assert torch.equal(gbuf.cpu(), torch.zeros(n) if dc else g)
        lr32 = float(cpu_ref.adam_constants(LR, 0.5, B1, B2, i)[0])
        W, M, V, stats, Ew, Em = replay(
            opt, *before[:1], g.double(), *before[1:], i + 1, 0.5,
            0.625 if clip else 1.0, mask.double(), lr32, offs, lens, adapt,
            chain)
        kw_, km, kv = w.cpu(), m.cpu(), v.cpu()
        for got, want, bound in ((kw_, W, Ew), (km, M, Em),
                                 (kv, V, SLACK * 7 * EPS * V)):
            excess = float(((got.double() - want).abs() - bound).max())
            assert excess <= 0, (i, excess)
        worst = max(worst, float(((kw_.double() - W).abs() / Ew.clamp_min(1e-300)).max()))
        assert torch.equal(sh.cpu().view(torch.int16),
                           kw_.to(torch.bfloat16).view(torch.int16))
        # the elementwise part, bit for bit
        if opt == "adam":
            cpu_ref.adam_step(rw, g, rm, rv, LR, 0.5, **hp, mask=mask,
                              offset=i, ema=re if ema else None,
                              ema_decay=D if ema else 0.0,
                              clip_coef=None if coef is None else coef.cpu())
            assert torch.equal(bits(kw_), bits(rw)), i
            assert torch.equal(bits(km), bits(rm)) and torch.equal(bits(kv), bits(rv))
            if ema:
                assert torch.equal(bits(e), bits(re))
        else:
            for t, (wn, un, r, Ewn, Eun, Er) in enumerate(stats):
                got = st[3 * t:3 * t + 3].tolist()
                assert got[2] == float(tab[t])
                assert abs(got[0] - wn) <= SLACK * Ewn * wn, (t, got)
                assert abs(got[1] - un) <= SLACK * Eun * un, (t, got)
                assert abs(got[2] - r) <= SLACK * Er * r, (t, got)
                assert (got[2] == 1.0) == (t == 1)
            if ema:  # fl(e - fl(w_e * fl(e - w'))), the same three roundings
                want = e_before - (e_before - kw_) * cpu_ref.ema_weight(D, i)
                assert torch.equal(bits(e), bits(want))
        if not ema:
            assert torch.equal(bits(e), bits(e_before))
    assert all(bool((b[n:] == 7.5).all()) for b in buf.values())  # canaries
    print(f"{opt} n={n}: worst |dw| / bound {worst:.3f}, chain {chain}")


def test_lamb_is_reproducible(ext):
    offs, lens, adapt, w0, grads = layout(BIG)
    n = w0.numel()
    out = []
    for _ in range(2):
        w, g = w0.cuda(), grads[0].cuda()
        m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        tab, st = Fx.lamb_step(w, g, m, v, LR, 0.5, B1, B2, AEPS, WD, offs,
                               lens, adapt, drop_connect_keep=KEEP, seed=SEED)
        out.append((tab, st, w, m, v))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(*out))
    assert float(out[0][0][0]) != 1.0


# -- trainer runs -----------------------------------------------------------------------

B, STEPS = 64, 3


def trainer_run(tmp_path, tag, opt, scope, *extra):
    from distributedmnist_amd import _C
    from distributedmnist_amd.engine.graphstep import GraphedStep
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    argv = ["--synthetic_data", "--model", "lenet", "--batch_size", str(B),
            "--max_steps", str(STEPS), "--optimizer", opt, "--weight_decay",
            "1e-2", "--moving_average_decay", "0.9", "--clip_grad_norm", "1",
            "--save_interval_secs", "100000", "--train_dir",
            str(tmp_path / tag), *extra]
    argv += ["--hip_graph", "off"] if scope == "eager" else []
    flags = build_train_parser().parse_args(argv)
    try:
        t = Trainer(flags, device=torch.device("cuda:0"))
        ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
        if scope == "split":
            t._graph = GraphedStep(t, (B, 28, 28, 1), split=True)
            t._graph_tried = True
        before = None
        for _ in range(STEPS):
            x, y = ds.next_batch(B)
            before = [b.double().cpu() for b in (
                t.fp.flat_master, t.flat_adam_m, t.flat_adam_v)]
            _, loss, _, _ = t.graph_or_eager_step(x, y)
            assert float(loss) == float(loss)
        torch.cuda.synchronize()
        assert (t._graph is not None) == (scope != "eager"), "capture must engage"
        state = [x.cpu() for x in (t.fp.flat_master, t.flat_adam_m,
                                   t.flat_adam_v, t.flat_ema)]
        # eager steps leave the aggregated gradient in the bucket
        return t, state, before, t.fp.flat_grad.double().cpu()
    finally:
        _C.ext().set_deterministic(False)


@pytest.mark.parametrize("opt", ["adam", "lamb"])
def test_trainer_scopes_agree_bitwise(tmp_path, ext, opt):
    """Eager, the full graph and the split graph: the same weights, moments
    and average.  Compared under --deterministic only: without it the
    backward kernels add the gradients with fp32 atomics, so two runs of one
    scope already differ and no bitwise comparison between scopes holds."""
    runs = {s: trainer_run(tmp_path, s, opt, s, "--deterministic")
            for s in ("eager", "full", "split")}
    t, state, before, grad = runs["eager"]
    assert bool(state[1].any()) and bool(state[2].any())
    assert not torch.equal(state[0], state[3])
    for s in ("full", "split"):
        assert all(torch.equal(bits(a), bits(b))
                   for a, b in zip(runs[s][1], state)), s
    if opt == "lamb":
        # (|w_t|, |u_t|, r_t) of the last update against its float64 replay
        fp = t.fp
        _, chain = ext.lamb_norm_plan(fp.flat_master.numel())
        ratios = t.trust_ratios()
        assert ratios == runs["split"][0].trust_ratios()
        lr32 = float(cpu_ref.adam_constants(
            t.flags.initial_learning_rate, 1.0, B1, B2, 0)[0])
        stats = replay("lamb", before[0], grad, *before[1:], STEPS, 1.0,
                       t.grad_norms()["clip_coef"], 1.0, lr32, fp.offsets,
                       fp.numels, t.lars_adapt, chain)[3]
        for name, (wn, un, r, Ewn, Eun, Er) in zip(fp.names, stats):
            got = ratios[name]
            assert abs(got[0] - wn) <= SLACK * Ewn * wn, (name, got)
            assert abs(got[1] - un) <= SLACK * Eun * un, (name, got)
            assert abs(got[2] - r) <= SLACK * Er * r, (name, got)
            assert (got[2] == 1.0) == name.endswith("_b")
