"""fp32 PyTorch reference implementations of every hot-path primitive.

These are (a) the CPU execution path (no GPU required — BASELINE config 1),
and (b) the numerics oracle the HIP/CDNA4 kernels are unit-tested against
(SURVEY.md section 4).  Layouts follow the reference model (TF NHWC / HWIO,
/root/reference/src/mnist.py:107-145): activations are NHWC, conv weights are
[KH, KW, Cin, Cout], fc weights are [in, out] with y = x @ W + b.

All functions are pure tensor->tensor (no autograd); autograd wiring lives in
ops/functional.py.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F


# ---------------------------------------------------------------------------
# conv 5x5 SAME + bias + ReLU + maxpool 2x2 s2, fused (fwd + bwd)
# Reference call sites: mnist.py:107-127 (conv/bias_add/relu/max_pool x2).
# ---------------------------------------------------------------------------

def conv_pool_fwd(x, w, b):
    """x: [N,H,W,Cin], w: [5,5,Cin,Cout], b: [Cout] ->
    (y: [N,H/2,W/2,Cout], argmax: [N,H/2,W/2,Cout] uint8 in 0..3)

    y = maxpool2x2(relu(conv2d_same(x, w) + b)); argmax records which of the
    2x2 window (r*2+c) won, for routing the pooled gradient back.
    """
    N, H, W, Cin = x.shape
    Cout = w.shape[3]
    xc = x.permute(0, 3, 1, 2)                       # NCHW
    wc = w.permute(3, 2, 0, 1)                       # [Cout,Cin,5,5]
    conv = F.conv2d(xc.float(), wc.float(), b.float(), padding=2)
    act = F.relu(conv)                               # [N,Cout,H,W]
    # maxpool 2x2 stride 2 with argmax
    pooled, idx = F.max_pool2d(act, 2, 2, return_indices=True)
    # idx is flat index into H*W; convert to 0..3 position within the window
    Ho, Wo = pooled.shape[2], pooled.shape[3]
    ar = torch.arange(Ho, device=x.device).view(1, 1, Ho, 1)
    ac = torch.arange(Wo, device=x.device).view(1, 1, 1, Wo)
    r = idx // W - ar * 2
    c = idx % W - ac * 2
    amax = (r * 2 + c).to(torch.uint8)               # [N,Cout,Ho,Wo]
    # liveness rides in the argmax byte (matches the HIP kernels): 7 marks
    # a dead window (relu zeroed all four) so pooled-consumer backward
    # kernels need no y read
    amax = torch.where(pooled > 0, amax,
                       torch.tensor(7, dtype=torch.uint8))
    y = pooled.permute(0, 2, 3, 1).contiguous()      # NHWC
    amax = amax.permute(0, 2, 3, 1).contiguous()
    return y, amax


def conv_pool_bwd(dy, x, w, y, amax):
    """Backward of conv_pool_fwd. Returns (dx, dw, db).

    dy, y, amax: [N,Ho,Wo,Cout]; x: [N,H,W,Cin]; w: [5,5,Cin,Cout].
    ReLU mask: the pooled max is the relu output at the argmax position, so
    grad passes iff y > 0.
    """
    N, Ho, Wo, Cout = dy.shape
    H, W = Ho * 2, Wo * 2
    Cin = x.shape[3]
    # route pooled grad (masked by relu) back to the argmax position
    g = (dy * (y > 0)).permute(0, 3, 1, 2).float()   # [N,Cout,Ho,Wo]
    # clamp the dead-window marker (7) to a valid position: its g is zero
    # by the relu mask, so the scatter target is irrelevant but must be
    # in-bounds
    am = amax.permute(0, 3, 1, 2).long().clamp(max=3)
    dact = x.new_zeros((N, Cout, H, W), dtype=torch.float32)
    ar = torch.arange(Ho, device=x.device).view(1, 1, Ho, 1)
    ac = torch.arange(Wo, device=x.device).view(1, 1, 1, Wo)
    rows = ar * 2 + am // 2
    cols = ac * 2 + am % 2
    flat = (rows * W + cols)
    dact.view(N, Cout, H * W).scatter_(2, flat.view(N, Cout, -1),
                                       g.view(N, Cout, -1))
    xc = x.permute(0, 3, 1, 2).float()               # [N,Cin,H,W]
    wc = w.permute(3, 2, 0, 1).float()               # [Cout,Cin,5,5]
    dxc = torch.nn.grad.conv2d_input(xc.shape, wc, dact, padding=2)
    dwc = torch.nn.grad.conv2d_weight(xc, wc.shape, dact, padding=2)
    db = dact.sum(dim=(0, 2, 3))
    dx = dxc.permute(0, 2, 3, 1).contiguous().to(x.dtype)
    dw = dwc.permute(2, 3, 1, 0).contiguous()        # [5,5,Cin,Cout] fp32
    return dx, dw, db


# ---------------------------------------------------------------------------
# Linear (+ bias [+ ReLU] [+ dropout]) — mnist.py:136-145
# ---------------------------------------------------------------------------

def linear_fwd(x, w, b, relu: bool = False):
    """x: [B,K], w: [K,N], b: [N] -> y: [B,N] (= relu(x@w+b) if relu)."""
    y = x.float() @ w.float() + b.float()
    if relu:
        y = F.relu(y)
    return y.to(x.dtype)


def linear_bwd(dy, x, w, y=None, relu: bool = False):
    """Returns (dx, dw fp32, db fp32). If relu, y (post-relu) masks dy."""
    dyf = dy.float()
    if relu:
        dyf = dyf * (y > 0)
    dx = (dyf @ w.float().t()).to(x.dtype)
    dw = x.float().t() @ dyf
    db = dyf.sum(dim=0)
    return dx, dw, db


def dropout_fwd(x, p_drop: float, gen: torch.Generator | None = None):
    """TF-style dropout (mnist.py:139-140): keep with prob 1-p, scale by
    1/(1-p). Returns (y, mask bool)."""
    keep = 1.0 - p_drop
    # generator lives on CPU; sample there and move (device-agnostic ref)
    mask = (torch.rand(x.shape, device="cpu", dtype=torch.float32,
                       generator=gen) < keep).to(x.device)
    y = x * mask.to(x.dtype) / keep
    return y.to(x.dtype), mask


def dropout_bwd(dy, mask, p_drop: float):
    keep = 1.0 - p_drop
    return (dy * mask.to(dy.dtype) / keep).to(dy.dtype)


# ---------------------------------------------------------------------------
# Fused softmax cross-entropy (+ accuracy): mnist.py:149-164
# ---------------------------------------------------------------------------

def softmax_xent_fwd(logits, labels):
    """logits: [B,C], labels: [B] int64.

    Returns (loss_mean fp32 scalar, correct_count fp32 scalar, dlogits
    [B,C] in logits.dtype).  dlogits = (softmax - onehot)/B — precomputed in
    the forward since the backward needs nothing else (single fused kernel on
    GPU; logsumexp trick).
    """
    lf = logits.float()
    m = lf.max(dim=1, keepdim=True).values
    z = lf - m
    ez = z.exp()
    se = ez.sum(dim=1, keepdim=True)
    logp = z - se.log()
    B = logits.shape[0]
    loss = -logp.gather(1, labels.view(-1, 1)).mean()
    p = ez / se
    dl = p
    dl.scatter_add_(1, labels.view(-1, 1), torch.full((B, 1), -1.0, device=logits.device))
    dl = (dl / B).to(logits.dtype)
    correct = (lf.argmax(dim=1) == labels).float().sum()
    return loss, correct, dl


def fc2_head(a1, w2, b2, labels, p_keep: float):
    """The fc2 layer of the training step in one piece: forward, softmax
    cross-entropy, fc2 dW and fc2 dX with the fc1 relu/dropout mask.

    a1: [B,K] post-relu/dropout activation, w2: [K,C], b2: [C], labels: [B].
    fp64 arithmetic with the GPU route's rounding points: the logits and
    dlogits are rounded to a1.dtype, db2 sums the unrounded dlogits, the mask
    is a1 > 0 and kept gradients are scaled by 1/p_keep.

    Returns (loss, correct, dyeff1 [B,K] in a1.dtype, dw2 [K,C], db1 [K],
    db2 [C]); the scalars and the three sums are fp64.
    """
    B = a1.shape[0]
    af, wf = a1.double(), w2.double()
    logits = (af @ wf + b2.double()).to(a1.dtype).double()
    z = logits - logits.max(dim=1, keepdim=True).values
    ez = z.exp()
    se = ez.sum(dim=1, keepdim=True)
    onehot = torch.zeros_like(ez).scatter_(1, labels.view(-1, 1), 1.0)
    loss = -((z - se.log()) * onehot).sum() / B
    correct = (logits.argmax(dim=1) == labels).double().sum()
    d = (ez / se - onehot) / B
    db2 = d.sum(dim=0)
    dl = d.to(a1.dtype).double()
    dw2 = af.t() @ dl
    g = (dl @ wf.t()) * (a1 > 0) / p_keep
    db1 = g.sum(dim=0)
    return loss, correct, g.to(a1.dtype), dw2, db1, db2


# ---------------------------------------------------------------------------
# Fused SGD apply (+ drop-connect): distributed_train.py:176,414-416
# ---------------------------------------------------------------------------

def sgd_step(master, grad, lr: float, grad_scale: float = 1.0,
             drop_connect_keep: float | None = None,
             gen: torch.Generator | None = None, shadow=None,
             momentum=None, mu: float = 0.0, ema=None,
             ema_decay: float = 0.0, offset: int = 0, clip_coef=None,
             lars_tab=None, offsets=None, numels=None):
    """In-place w -= lr * grad_scale * (g or momentum-filtered g).

    lars_tab (with offsets, numels; not with clip_coef): lars_norm()'s table.
    Tensor t = [offsets[t], offsets[t] + numels[t]) does g = tab[2t]*g, then
    the drop-connect mask, then the unmasked decay g += tab[2t + 1]*w (times
    grad_scale: the table's decay entry is in units of the SUM over
    contributors), then momentum.

    clip_coef: optional one-element fp32 tensor (grad_norm()'s stats[1:2]);
    the gradient is multiplied by it first, before the drop-connect mask and
    before momentum: v = mu*v + coef*g.

    drop_connect_keep: if set, per-element Bernoulli(keep) mask on the grad
    (reference drop_connect: grad * mask, NO rescale —
    distributed_train.py:414-416).
    momentum/mu: optional heavyweight-ball momentum v = mu*v + g; w -= lr*v
    (the reference used plain GradientDescentOptimizer; momentum is the
    north-star's optional extension).
    shadow: optional flat low-precision copy refreshed after the update.
    ema/ema_decay/offset: optional moving average of the weights
    (TensorFlow's ExponentialMovingAverage with num_updates): update
    k = offset + 1 does e -= (1 - d_k)*(e - w_new), d_k = min(ema_decay,
    (1 + k)/(10 + k)), everything in fp32.
    """
    g = grad.float() * grad_scale
    if clip_coef is not None:
        if lars_tab is not None:
            raise ValueError("sgd_step: lars_tab and clip_coef are mutually "
                             "exclusive")
        g = g * clip_coef.float().reshape(())
    decay = None
    if lars_tab is not None:
        segs = torch.repeat_interleave(
            torch.arange(len(offsets), device=g.device),
            torch.tensor([int(m) for m in numels], device=g.device))
        if segs.numel() != g.numel() or list(offsets) != [
                sum(numels[:i]) for i in range(len(numels))]:
            raise ValueError("sgd_step: the segments must tile [0, n) in "
                             "order")
        tab = lars_tab.float()
        g = g * tab[2 * segs]
        decay = (tab[2 * segs + 1] * grad_scale) * master
    if drop_connect_keep is not None:
        mask = (torch.rand(g.shape, device=g.device, dtype=torch.float32,
                           generator=gen) < drop_connect_keep).float()
        g = g * mask
    if decay is not None:
        g = g + decay
    if momentum is not None:
        momentum.mul_(mu).add_(g)
        g = momentum
    master.add_(g, alpha=-lr)
    if ema is not None:
        ema.sub_((ema - master) * ema_weight(ema_decay, offset))
    if shadow is not None:
        shadow.copy_(master.to(shadow.dtype))
    return master


def grad_norm(flat, offsets, numels, grad_scale: float, clip: float):
    """Per-tensor and global L2 norms of a flat fp32 gradient and the
    torch.nn.utils.clip_grad_norm_ coefficient -> fp32 `stats` [2 + segments]
    on flat's device, the layout of csrc/grad_norm.hip:

      stats[0]     = grad_scale * sqrt(sum of g^2)       (the global norm)
      stats[1]     = min(1, clip / (stats[0] + 1e-6))    (fp32 arithmetic)
      stats[2 + s] = grad_scale * sqrt(sum of g^2 over segment s)

    The sums of squares are taken per segment in float64 from the fp32
    values, the total is their float64 sum, the norms are rounded to fp32.
    `flat` is the SUM over contributors, grad_scale = 1 / contributors, so the
    norms are those of the averaged gradient.  The segments (offsets, numels)
    must tile [0, flat.numel()) in order; clip > 0, inf = never clip (the
    coefficient is then exactly 1)."""
    import numpy as np
    n = flat.numel()
    if flat.dtype != torch.float32 or flat.dim() != 1:
        raise ValueError("grad_norm: flat must be a 1-D fp32 tensor")
    if not (len(offsets) == len(numels) and len(offsets) >= 1):
        raise ValueError("grad_norm: one length per offset, at least one")
    at = 0
    for o, m in zip(offsets, numels):
        if o != at or m < 0:
            raise ValueError("grad_norm: the segments must tile [0, n) in "
                             "order")
        at += m
    if at != n:
        raise ValueError("grad_norm: the segments must tile [0, n) in order")
    if not clip > 0.0:  # also refuses nan
        raise ValueError(f"grad_norm: clip must be > 0, got {clip}")
    g = flat.detach().double()
    sq = [float((g[o:o + m] * g[o:o + m]).sum())
          for o, m in zip(offsets, numels)]
    total = 0.0
    for v in sq:
        total += v
    f32 = np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        norm = f32(float(grad_scale) * np.sqrt(total))
        coef = np.minimum(f32(1), f32(clip) / (norm + f32(1e-6)))
        if np.isnan(coef):
            coef = f32(1)  # fminf(1, nan)
    out = [norm, coef] + [f32(float(grad_scale) * np.sqrt(v)) for v in sq]
    return torch.tensor([float(v) for v in out], dtype=torch.float32,
                        device=flat.device)


def topk_ks(numels, ratio: float):
    """--grad_topk RATIO: pairs sent per tensor, min(n, max(1, ceil(RATIO *
    n))); an empty tensor sends none."""
    if not 0.0 < ratio <= 1.0:  # also refuses nan
        raise ValueError(f"topk_ks: ratio must lie in (0, 1], got {ratio}")
    return [min(int(n), max(1, math.ceil(ratio * int(n)))) for n in numels]


def topk_compress(g, r, offsets, numels, ks):
    """Top-k sparsification with error feedback, the contract of
    csrc/topk.hip.  a = r + g (one fp32 add per element); per segment the
    ks[t] elements first under "larger bits(a) & 0x7fffffff, then smaller
    index" are selected.  Returns (payload, dense): payload int32 [2][K], the
    selected global indices in ascending order per segment (segment t in the
    slots from sum(ks[:t])), then the bits of their a; dense = a where
    selected, 0 elsewhere.  r is updated in place: 0 where selected, a
    elsewhere.  Exact: integer compares only."""
    if g.dtype != torch.float32 or g.dim() != 1 or r.shape != g.shape:
        raise ValueError("topk_compress: g and r are 1-D fp32 of one length")
    if not len(offsets) == len(numels) == len(ks):
        raise ValueError("topk_compress: one length and one k per offset")
    a = r + g
    abits = a.view(torch.int32)
    keys = abits & 0x7FFFFFFF
    K = int(sum(ks))
    payload = torch.zeros(2, K, dtype=torch.int32, device=g.device)
    dense = torch.zeros_like(a)
    base = 0
    for o, m, k in zip(offsets, numels, ks):
        if not (0 <= k <= m and (k >= 1 or m == 0)):
            raise ValueError(f"topk_compress: k = {k} for {m} elements")
        if k == 0:
            continue
        # stable: equal keys keep their index order
        order = torch.sort(keys[o:o + m], descending=True, stable=True)[1]
        idx = torch.sort(order[:k])[0] + o
        payload[0, base:base + k] = idx.to(torch.int32)
        payload[1, base:base + k] = abits[idx]
        dense[idx] = a[idx]
        a[idx] = 0.0
        base += k
    r.copy_(a)
    return payload, dense


def topk_scatter(payloads, n: int):
    """The dense fp32 bucket [n] of the ranks' payloads (int32 [W][2][K]):
    zeros, then g[index] += value rank by rank in rank order (indices are
    unique within one rank), so every rank that runs this holds the same
    bits."""
    payloads = payloads.reshape(-1, 2, payloads.shape[-1])
    g = torch.zeros(n, dtype=torch.float32, device=payloads.device)
    for p in payloads:
        g[p[0].long()] += p[1].view(torch.float32)
    return g


LOWRANK_MAX_TENSORS = 4


def lowrank_plan(shapes, offsets, R: int):
    """--grad_lowrank R: which tensors of the bucket are compressed.  Returns
    [(index, offset, rows, cols)].  A tensor is viewed as [rows = numel /
    shape[-1]][cols = shape[-1]] and compressed iff it has at least 2 dims,
    rows % 16 == 0 == cols % 16, 64 <= rows <= 4096, 64 <= cols <= 512 and
    its bucket offset is a multiple of 4; every other tensor is sent dense,
    exactly, and has no residual."""
    if not 1 <= int(R) <= 16:
        raise ValueError(f"lowrank_plan: rank must lie in 1..16, got {R}")
    plan = []
    for i, (shape, off) in enumerate(zip(shapes, offsets)):
        if len(shape) < 2:
            continue
        cols = int(shape[-1])
        rows = int(math.prod(shape)) // max(cols, 1)
        if (rows % 16 == 0 and cols % 16 == 0 and 64 <= rows <= 4096
                and 64 <= cols <= 512 and int(off) % 4 == 0):
            plan.append((i, int(off), rows, cols))
    if len(plan) > LOWRANK_MAX_TENSORS:
        raise ValueError(f"--grad_lowrank supports at most "
                         f"{LOWRANK_MAX_TENSORS} compressed tensors, this "
                         f"model has {len(plan)}")
    return plan


def lowrank_q_init(plan, R: int, seed: int):
    """The start factors [Q of tensor 0 | Q of tensor 1 | ..], Q [cols][R]
    standard normal keyed on (seed, tensor index): built on the host, so
    every rank and every device holds the same bits."""
    qs = []
    for i, _, _, cols in plan:
        gen = torch.Generator().manual_seed(int(seed) * 1000003 + 7919 * i + 1)
        qs.append(torch.randn(cols, R, generator=gen).reshape(-1))
    return torch.cat(qs)


def lowrank_orth(P):
    """Modified Gram-Schmidt of the columns of P, in column order, each column
    divided by (its 2-norm + 1e-8) as in torch's PowerSGD hook, so a zero
    column stays zero.  The divided column q is a little short of unit length,
    so the projection of the later columns divides by q.q: rest -= (q.rest /
    q.q) q.  (The hook leaves that division out; 2e-8 of every projection
    then stays behind, and the same 1e-8 blows a dependent column, which is
    nothing but that remainder, up to a norm of order one.)
    Before a column is divided it is projected once more against all
    finished columns: in fp32 a dependent column is rounding noise far above
    1e-8, and without the second pass it would become a unit vector that is
    not orthogonal to the others, so that P P^T were no projector."""
    P = P.clone()
    qqs = []
    for i in range(P.shape[1]):
        if i > 0:
            done, qq = P[:, :i], torch.stack(qqs)
            dots = (done * P[:, i:i + 1]).sum(0)
            P[:, i] -= (done * torch.where(qq > 0, dots / qq,
                                           torch.zeros_like(dots))).sum(1)
        P[:, i] = P[:, i] / (torch.linalg.vector_norm(P[:, i]) + 1e-8)
        q = P[:, i:i + 1]
        qqs.append((q * q).sum())
        if i + 1 < P.shape[1]:
            dots = (q * P[:, i + 1:]).sum(0)
            P[:, i + 1:] -= torch.where(qqs[i] > 0, dots / qqs[i],
                                        torch.zeros_like(dots)) * q
    return P


def lowrank_step(G, E, Q, reduce=None):
    """One PowerSGD step (Vogels et al. 2019) of one [rows][cols] tensor, the
    contract of csrc/lowrank.hip, in the dtype of its inputs:
      M = G + E;  P = M Q (summed over ranks);  P^ = lowrank_orth(P);
      Q_r = M^T P^ (summed over ranks: Q_S);  bucket = P^ Q_S^T, the SUM of
      the ranks' approximations;  E' = M - P^ Q_r^T, this rank's own share.
    `reduce` sums a tensor over the ranks (None: one rank).  Returns (bucket,
    E', Q_S, P^); Q_S is the next step's Q."""
    M = G + E
    P = M @ Q
    if reduce is not None:
        P = reduce(P)
    Ph = lowrank_orth(P)
    Qr = M.t() @ Ph
    Qs = reduce(Qr) if reduce is not None else Qr
    return Ph @ Qs.t(), M - Ph @ Qr.t(), Qs, Ph


def lars_norm(master, flat, offsets, numels, adapt_mask: int,
              grad_scale: float, eta: float, wd: float, clip: float = 0.0):
    """LARS trust ratios (You, Gitman, Ginsburg 2017) of the flat fp32
    `master` and the flat fp32 gradient `flat` (the SUM over contributors,
    grad_scale = s = 1 / contributors), the layout of csrc/lars.hip:

      lars_tab[2t]     = a_t = ratio_t * coef
      lars_tab[2t + 1] = d_t = ratio_t * wd / s     (0 if t is not adaptive)
      lars_stats[3t:]  = (wn_t, gn_t, ratio_t)

    wn_t = sqrt(sum w^2), gn_t = coef * (s * sqrt(sum g^2)), and for the
    tensors whose bit is set in adapt_mask ratio_t = eta * wn_t / (gn_t + wd *
    wn_t) when both norms are > 0; every other ratio is 1.  coef is
    grad_norm()'s clip coefficient for clip > 0 and exactly 1 for clip = 0
    (no clipping).  Sums in float64 from the fp32 values, everything after
    them in fp32 in the order written here.  Returns (lars_tab [32], lars_stats
    [3 * segments], clip_stats [2 + segments] or None)."""
    import numpy as np
    f32 = np.float32
    if master.shape != flat.shape or master.dtype != torch.float32:
        raise ValueError("lars_norm: master and flat are 1-D fp32 tensors of "
                         "one length")
    if not (eta > 0.0 and math.isfinite(eta)):
        raise ValueError(f"lars_norm: eta must be finite and > 0, got {eta}")
    if not (wd >= 0.0 and math.isfinite(wd)):
        raise ValueError(f"lars_norm: wd must be finite and >= 0, got {wd}")
    if not (grad_scale > 0.0 and math.isfinite(grad_scale)):
        raise ValueError("lars_norm: grad_scale must be finite and > 0")
    if not clip >= 0.0:
        raise ValueError(f"lars_norm: clip must be 0 (off) or > 0, got {clip}")
    ns = len(offsets)
    if ns > 16 or not 0 <= adapt_mask < (1 << ns):
        raise ValueError("lars_norm: at most 16 segments, one mask bit each")
    # the table checks, the float64 segment sums and the coefficient
    gstats = grad_norm(flat, offsets, numels, grad_scale,
                       clip if clip > 0 else math.inf)
    coef = f32(gstats[1].item()) if clip > 0 else f32(1)
    w = master.detach().double()
    s, eta32, wd32 = f32(grad_scale), f32(eta), f32(wd)
    tab = np.zeros(32, dtype=np.float32)
    tab[0::2] = 1.0
    stats = np.zeros(3 * ns, dtype=np.float32)
    for t, (o, m) in enumerate(zip(offsets, numels)):
        wn = f32(np.sqrt(float((w[o:o + m] * w[o:o + m]).sum())))
        gn = f32(coef * f32(gstats[2 + t].item()))
        adaptive = bool((adapt_mask >> t) & 1)
        ratio = f32(1)
        if adaptive and wn > 0 and gn > 0:
            ratio = f32(f32(eta32 * wn) / f32(gn + f32(wd32 * wn)))
        tab[2 * t] = f32(ratio * coef)
        tab[2 * t + 1] = f32(f32(ratio * wd32) / s) if adaptive else f32(0)
        stats[3 * t:3 * t + 3] = (wn, gn, ratio)
    dev = flat.device
    return (torch.from_numpy(tab).to(dev), torch.from_numpy(stats).to(dev),
            gstats if clip > 0 else None)


# ---------------------------------------------------------------------------
# Adam / AdamW and LAMB (--optimizer; csrc/adam.hip).  Every fp32 operation
# below is one torch op or one numpy.float32 op, in the kernels' order.
# ---------------------------------------------------------------------------

def adam_constants(lr: float, grad_scale: float, beta1: float, beta2: float,
                   offset: int):
    """(lr, c1, c2) of update k = offset + 1 as the kernels form them, in
    numpy.float32: lr = fl(lr * s) * contributors, c = 1 - beta^k as the
    correctly rounded -expm1 of the fp32 product k * ln(beta), ln(beta)
    rounded once from double."""
    import numpy as np
    f32 = np.float32
    contrib = f32(round(1.0 / grad_scale))
    k = f32(int(offset) + 1)
    with np.errstate(invalid="ignore"):
        c = [f32(-np.expm1(np.float64(
            k * f32(math.log(b) if b > 0 else -math.inf))))
            for b in (beta1, beta2)]
    return f32(lr * grad_scale) * contrib, c[0], c[1]


def _adam_check(master, beta1, beta2, eps, wd, grad_scale):
    if master.dtype != torch.float32 or master.dim() != 1:
        raise ValueError("adam: master must be a 1-D fp32 tensor")
    if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
        raise ValueError("adam: beta1 and beta2 must lie in [0, 1)")
    if not (eps > 0.0 and math.isfinite(eps)):
        raise ValueError(f"adam: eps must be finite and > 0, got {eps}")
    if not (wd >= 0.0 and math.isfinite(wd)):
        raise ValueError(f"adam: wd must be finite and >= 0, got {wd}")
    if not 0.0 < grad_scale <= 1.0:
        raise ValueError("adam: grad_scale must be 1 / contributors")


def _f32(x) -> float:
    import numpy as np
    return float(np.float32(x))


def _adam_decay(master, wd, offsets, numels, adapt_mask):
    """wd on the tensors whose bit is set in adapt_mask, 0 elsewhere."""
    if sum(int(m) for m in numels) != master.numel():
        raise ValueError("adam: the segments must tile [0, n) in order")
    per = torch.tensor([_f32(wd) if (adapt_mask >> t) & 1 else 0.0
                        for t in range(len(offsets))], dtype=torch.float32)
    return torch.repeat_interleave(per, torch.tensor(
        [int(m) for m in numels])).to(master.device)


def adam_moments(grad, m, v, grad_scale, beta1, beta2, eps, c1, c2,
                 clip_coef=None, mask=None):
    """m, v in place from gh = ((g * s) * coef) * mask; returns
    u = (m / c1) / (sqrt(v / c2) + eps)."""
    gh = grad.float() * _f32(grad_scale)
    gh = gh * (clip_coef.float().reshape(()) if clip_coef is not None else 1.0)
    if mask is not None:
        gh = gh * mask
    m.mul_(_f32(beta1)).add_(gh * _f32(1.0 - beta1))
    v.mul_(_f32(beta2)).add_((gh * gh) * _f32(1.0 - beta2))
    return adam_u(m, v, eps, c1, c2)


def adam_u(m, v, eps, c1, c2):
    # full tensors as divisors (torch may divide by a scalar through its
    # reciprocal, which rounds twice) and numpy's correctly rounded sqrt
    # (torch's vectorized CPU sqrt is not, in about 1 value of 100)
    import numpy as np
    vh = v / torch.full_like(v, float(c2))
    root = torch.from_numpy(np.sqrt(vh.cpu().numpy())).to(v.device)
    return (m / torch.full_like(m, float(c1))) / (root + _f32(eps))


def _adam_publish(master, ema, ema_decay, offset, shadow):
    if ema is not None:
        ema.sub_((ema - master) * ema_weight(ema_decay, offset))
    if shadow is not None:
        shadow.copy_(master.to(shadow.dtype))


def _dc_mask(n, drop_connect_keep, gen, mask, device):
    if mask is None and drop_connect_keep is not None:
        mask = (torch.rand(n, device=device, dtype=torch.float32,
                           generator=gen) < drop_connect_keep).float()
    return mask


def adam_step(master, grad, m, v, lr: float, grad_scale: float = 1.0,
              beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
              wd: float = 0.0, offsets=None, numels=None, adapt_mask: int = 0,
              drop_connect_keep=None, gen=None, mask=None, shadow=None,
              ema=None, ema_decay: float = 0.0, offset: int = 0,
              clip_coef=None):
    """In-place Adam / AdamW update k = offset + 1 of the flat fp32 `master`
    with the aggregated gradient `grad` (the SUM over contributors, grad_scale
    = s = 1 / contributors):

      gh = coef * s * g, then the drop-connect mask
      m = b1*m + (1 - b1)*gh          v = b2*v + (1 - b2)*gh^2
      u = (m / (1 - b1^k)) / (sqrt(v / (1 - b2^k)) + eps)
      w -= lr * (u + wd_t * w)        wd_t = wd on the tensors of adapt_mask

    then the moving average and the shadow as sgd_step does.  mask: an
    explicit keep mask instead of one drawn from `gen`."""
    _adam_check(master, beta1, beta2, eps, wd, grad_scale)
    offsets = [0] if offsets is None else offsets
    numels = [master.numel()] if numels is None else numels
    lr32, c1, c2 = adam_constants(lr, grad_scale, beta1, beta2, offset)
    mask = _dc_mask(master.numel(), drop_connect_keep, gen, mask,
                    master.device)
    u = adam_moments(grad, m, v, grad_scale, beta1, beta2, eps, c1, c2,
                     clip_coef, mask)
    u = u + _adam_decay(master, wd, offsets, numels, adapt_mask) * master
    master.sub_(u * float(lr32))
    _adam_publish(master, ema, ema_decay, offset, shadow)
    return master


def lamb_moments(master, grad, m, v, grad_scale: float, beta1: float,
                 beta2: float, eps: float, wd: float, offsets, numels,
                 adapt_mask: int, offset: int = 0, clip_coef=None,
                 drop_connect_keep=None, gen=None, mask=None):
    """LAMB pass 1: m, v in place (adam_step's), then per tensor the norms of
    the master and of u_t = u + wd_t * w (sums in float64 from the fp32
    values) and r_t = |w_t| / |u_t| for the tensors of adapt_mask with both
    norms > 0, else 1.  Returns (lamb_tab [16], lamb_stats [3 * segments] =
    (|w_t|, |u_t|, r_t))."""
    import numpy as np
    f32 = np.float32
    _adam_check(master, beta1, beta2, eps, wd, grad_scale)
    _, c1, c2 = adam_constants(0.0, grad_scale, beta1, beta2, offset)
    mask = _dc_mask(master.numel(), drop_connect_keep, gen, mask,
                    master.device)
    u = adam_moments(grad, m, v, grad_scale, beta1, beta2, eps, c1, c2,
                     clip_coef, mask)
    u = u + _adam_decay(master, wd, offsets, numels, adapt_mask) * master
    tab = np.ones(16, dtype=np.float32)
    stats = np.zeros(3 * len(offsets), dtype=np.float32)
    u64, w64 = u.double(), master.detach().double()
    for t, (o, n) in enumerate(zip(offsets, numels)):
        wn = f32(np.sqrt(float((w64[o:o + n] * w64[o:o + n]).sum())))
        un = f32(np.sqrt(float((u64[o:o + n] * u64[o:o + n]).sum())))
        if (adapt_mask >> t) & 1 and wn > 0 and un > 0:
            tab[t] = wn / un
        stats[3 * t:3 * t + 3] = (wn, un, tab[t])
    dev = master.device
    return torch.from_numpy(tab).to(dev), torch.from_numpy(stats).to(dev)


def lamb_apply(master, m, v, lamb_tab, lr: float, grad_scale: float,
               beta1: float, beta2: float, eps: float, wd: float, offsets,
               numels, adapt_mask: int, offset: int = 0, shadow=None,
               ema=None, ema_decay: float = 0.0):
    """LAMB pass 2: w -= (lr * r_t) * u_t with u_t recomputed from the
    moments lamb_moments left; then the moving average and the shadow."""
    _adam_check(master, beta1, beta2, eps, wd, grad_scale)
    lr32, c1, c2 = adam_constants(lr, grad_scale, beta1, beta2, offset)
    u = adam_u(m, v, eps, c1, c2)
    u = u + _adam_decay(master, wd, offsets, numels, adapt_mask) * master
    lr_t = torch.repeat_interleave(
        lamb_tab.float().cpu()[:len(offsets)] * float(lr32),
        torch.tensor([int(n) for n in numels])).to(master.device)
    master.sub_(u * lr_t)
    _adam_publish(master, ema, ema_decay, offset, shadow)
    return master


# ---------------------------------------------------------------------------
# Muon (--optimizer muon; csrc/muon.hip): Nesterov momentum whose per-matrix
# update is replaced by its Newton-Schulz orthogonalisation.  The rounding
# points are the kernels': X, G and P are bf16, products take bf16 operands
# and accumulate in fp32, the polynomial and a*X + X P are fp32 on the
# accumulator before the one rounding; the elementwise parts are one torch op
# per fp32 operation, in the kernels' order.
# ---------------------------------------------------------------------------
MUON_ABC = (3.4445, -4.7750, 2.0315)


def _bf16(x):
    return x.to(torch.bfloat16).float()


def muon_orthogonalize(x, iters: int = 5):
    """`iters` Newton-Schulz iterations of the [rows][cols] matrix `x`
    (fp32 or bf16) -> bf16, the arithmetic of csrc/muon.hip:

      X = bf16(x), s = 1 / (|x|_F + 1e-7)   (the sum in float64, then fp32)
      G = bf16(sc^2 * X^T X), P = bf16(b*G + c * G G),
      X = bf16(sc * (a*X + X P))

    with sc = s in the first iteration and 1 after it, so that X0 = s * X is
    never rounded on its own.  The Gram matrix is on the column side; the
    polynomial is odd, so this is right for rows < cols too."""
    import numpy as np
    f32 = np.float32
    if x.dim() != 2 or not iters >= 1:
        raise ValueError("muon_orthogonalize: x is a matrix, iters >= 1")
    a, b, c = (_f32(v) for v in MUON_ABC)
    xf = x.detach().float()
    norm = f32(np.sqrt(float((xf.double() * xf.double()).sum())))
    sc = float(f32(1) / (norm + f32(1e-7)))
    X = _bf16(xf)
    for _ in range(int(iters)):
        G = _bf16((X.t() @ X) * _f32(sc * sc))
        P = _bf16(G * b + (G @ G) * c)
        X = _bf16((X * a + X @ P) * sc)
        sc = 1.0
    return X.to(torch.bfloat16)


def muon_scale(rows: int, cols: int) -> float:
    """0.2 * sqrt(max(rows, cols)): the update RMS of Adam, in fp32."""
    return _f32(0.2 * math.sqrt(max(rows, cols)))


def muon_step(master, grad, mom, lr: float, grad_scale: float = 1.0,
              mu: float = 0.95, wd: float = 0.0, offsets=None, numels=None,
              cols=None, adapt_mask: int = 0, drop_connect_keep=None,
              gen=None, mask=None, shadow=None, ema=None,
              ema_decay: float = 0.0, offset: int = 0, clip_coef=None,
              iters: int = 5):
    """In-place Muon update k = offset + 1 of the flat fp32 `master` with the
    aggregated gradient `grad` (the SUM over contributors, grad_scale = s =
    1 / contributors) and the momentum buffer `mom`:

      gh = coef * s * g, then the drop-connect mask
      v = mu*v + gh                 u = gh + mu*v
      weight tensor t (bit t of adapt_mask), viewed [numel / cols[t]][cols[t]]:
        w = w*(1 - lr*wd) - (lr * muon_scale(rows, cols)) * orthogonalize(u)
      bias: w -= lr*v

    then the moving average and the shadow as sgd_step does."""
    import numpy as np
    f32 = np.float32
    if master.dtype != torch.float32 or master.dim() != 1:
        raise ValueError("muon: master must be a 1-D fp32 tensor")
    if not 0.0 <= mu < 1.0:
        raise ValueError(f"muon: mu must lie in [0, 1), got {mu}")
    if not (wd >= 0.0 and math.isfinite(wd)):
        raise ValueError(f"muon: wd must be finite and >= 0, got {wd}")
    if not 0.0 < grad_scale <= 1.0:
        raise ValueError("muon: grad_scale must be 1 / contributors")
    offsets = [0] if offsets is None else offsets
    numels = [master.numel()] if numels is None else numels
    if sum(int(m) for m in numels) != master.numel():
        raise ValueError("muon: the segments must tile [0, n) in order")
    lr32 = f32(lr * grad_scale) * f32(round(1.0 / grad_scale))
    decay = float(f32(1) - lr32 * f32(wd))
    mask = _dc_mask(master.numel(), drop_connect_keep, gen, mask,
                    master.device)
    gh = grad.float() * _f32(grad_scale)
    gh = gh * (clip_coef.float().reshape(()) if clip_coef is not None else 1.0)
    if mask is not None:
        gh = gh * mask
    mom.mul_(_f32(mu)).add_(gh)
    u = gh + mom * _f32(mu)
    for t, (o, n) in enumerate(zip(offsets, numels)):
        w = master[o:o + n]
        if (adapt_mask >> t) & 1:
            c = int(cols[t])
            x = muon_orthogonalize(u[o:o + n].view(n // c, c), iters)
            step = float(lr32 * f32(muon_scale(n // c, c)))
            w.mul_(decay).sub_(x.float().reshape(-1) * step)
        else:
            w.sub_(mom[o:o + n] * float(lr32))
    _adam_publish(master, ema, ema_decay, offset, shadow)
    return master


def ema_weight(ema_decay: float, offset: int) -> float:
    """1 - d_k of update k = offset + 1, in numpy.float32 (the arithmetic
    of sgd_step_kernel_ema)."""
    if not 0.0 <= ema_decay < 1.0:
        raise ValueError(f"ema_decay must lie in [0, 1), got {ema_decay}")
    import numpy as np
    k = np.float32(int(offset) + 1)
    d = min(np.float32(ema_decay),
            (np.float32(1) + k) / (np.float32(10) + k))
    return float(np.float32(1) - d)


# ---------------------------------------------------------------------------
# Device-resident input pipeline: stateless epoch permutation + batch gather.
# Bit-exact oracle of csrc/data_gather.hip (and the CPU / fp32-on-GPU path).
# All permutation arithmetic is unsigned mod 2^32.
# ---------------------------------------------------------------------------

_M32 = 0xFFFFFFFF


def _mix32(x):
    """murmur3 finalizer on python ints or uint64 numpy arrays (values kept
    below 2^32, so the 64-bit products never overflow before masking)."""
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & _M32
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & _M32
    return x ^ (x >> 16)


def feistel_perm(n: int, seed: int, epoch: int, p):
    """Cycle-walking 4-round Feistel permutation of [0, n) keyed on
    (64-bit seed, epoch).  p: int array of positions in [0, n) -> int64
    array of sample indices.  Epoch 0 is the identity (first epoch
    unshuffled, as data/mnist_data.py DataSet)."""
    import numpy as np
    p = np.asarray(p, dtype=np.int64)
    if p.size and not (0 <= p.min() and p.max() < n):
        raise ValueError(f"positions must lie in [0, {n})")
    if epoch == 0:
        return p.copy()
    seed &= 0xFFFFFFFFFFFFFFFF
    base = _mix32((seed & _M32) ^ _mix32(((seed >> 32) + 0x9E3779B9) & _M32))
    keys = [_mix32((base + (epoch & _M32) * 0x9E3779B1 + r) & _M32)
            for r in range(4)]
    bits = max(2, (n - 1).bit_length())
    bits += bits & 1
    h = np.uint64(bits // 2)
    mask = np.uint64((1 << (bits // 2)) - 1)
    m32 = np.uint64(_M32)

    def enc(v):
        L, R = v >> h, v & mask
        for k in keys:
            f = _mix32((R * np.uint64(0x9E3779B1) + np.uint64(k)) & m32)
            L, R = R, L ^ (f & mask)
        return (L << h) | R

    v = enc(p.astype(np.uint64))
    out = v >= np.uint64(n)
    while out.any():
        v[out] = enc(v[out])
        out = v >= np.uint64(n)
    return v.astype(np.int64)


def batch_indices(n: int, batch_size: int, seed: int, step: int):
    """Sample indices of the batch at `step`: spe = n // B batches per epoch
    (the n % B tail is dropped, as DataSet.next_batch drops it), epoch =
    step // spe, sample j = perm(epoch, (step % spe) * B + j)."""
    import numpy as np
    if not 1 <= batch_size <= n:
        raise ValueError(f"batch size {batch_size} must be in [1, N={n}]")
    if step < 0:
        raise ValueError("step must be >= 0")
    spe = n // batch_size
    epoch, pos = divmod(int(step), spe)
    p = pos * batch_size + np.arange(batch_size, dtype=np.int64)
    return feistel_perm(n, seed, epoch, p)


# -- affine augmentation (integer only; csrc/data_gather.hip mirrors it) -----
#
# A transform table is int32 [T, 6]: rows (a00, a01, a10, a11, t0, t1) in
# Q16, the INVERSE map (output pixel -> source position) about the image
# centre (13.5, 13.5):
#
#   src_col = 13.5 + a00 (c - 13.5) + a01 (r - 13.5) + t0
#   src_row = 13.5 + a10 (c - 13.5) + a11 (r - 13.5) + t1
#
# evaluated in Q17 on the doubled coordinates uc = 2c - 27, ur = 2r - 27 so
# that the half-pixel centre stays an integer.  The bilinear weights keep 8
# fractional bits; pixels outside the image are background byte 0.

AUG_ONE = 1 << 16
AUG_IDENTITY = (AUG_ONE, 0, 0, AUG_ONE, 0, 0)
AUG_MAX_A = 4 * AUG_ONE     # |a| bound the builder guarantees
AUG_MAX_T = 64 * AUG_ONE    # |t| bound the builder guarantees
_SIDE = 28


def augment_table(T: int, seed: int, shift_px: float = 0.0,
                  rotate_deg: float = 0.0, scale_frac: float = 0.0):
    """Seeded table of T random inverse affine maps -> int32 numpy [T, 6].
    Angle uniform in +-rotate_deg, scale log-uniform in [1/(1+scale_frac),
    1+scale_frac], translation uniform real in +-shift_px per axis; each
    entry is the inverse of rotate o scale (plus the translation of the
    source position), rounded to nearest.  All-zero magnitudes give the
    identity everywhere.  Arguments that could leave |a| <= 4 or |t| <= 64
    (in pixels) are rejected: inside those bounds the Q17 coordinates of
    affine_warp_u8 cannot overflow int32."""
    import numpy as np
    T = int(T)
    if T < 1:
        raise ValueError("augment_table: T must be >= 1")
    for name, v, hi in (("shift_px", shift_px, 64.0),
                        ("rotate_deg", rotate_deg, 180.0),
                        ("scale_frac", scale_frac, 3.0)):
        if not (0.0 <= float(v) <= hi):  # NaN fails both compares
            raise ValueError(f"augment_table: {name}={v} outside [0, {hi}]")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    rng = np.random.RandomState([seed & _M32, seed >> 32, 0xA0F1])
    theta = np.deg2rad(rng.uniform(-rotate_deg, rotate_deg, size=T))
    ls = np.log1p(float(scale_frac))
    inv_s = np.exp(-rng.uniform(-ls, ls, size=T))
    t = rng.uniform(-shift_px, shift_px, size=(T, 2))
    co, si = np.cos(theta) * inv_s, np.sin(theta) * inv_s
    # inverse of s*R(theta) is (1/s)*R(-theta)
    tab = np.stack([co, si, -si, co, t[:, 0], t[:, 1]], axis=1) * AUG_ONE
    tab = np.rint(tab).astype(np.int64)
    assert np.abs(tab[:, :4]).max() <= AUG_MAX_A
    assert np.abs(tab[:, 4:]).max() <= AUG_MAX_T
    return tab.astype(np.int32)


def aug_indices(T: int, seed: int, step: int, b: int):
    """Table row of batch position j at `step` -> int64 numpy [b] in [0, T):
    a pure function of (seed, step, j) that takes the full 64-bit step.
    Keyed on the batch POSITION, not on the sample index, so an image meets
    a different transform in every epoch."""
    import numpy as np
    T, step = int(T), int(step)
    if T < 1:
        raise ValueError("aug_indices: T must be >= 1")
    if step < 0:
        raise ValueError("step must be >= 0")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    base = _mix32((seed & _M32) ^ _mix32(((seed >> 32) + 0x9E3779B9) & _M32))
    lo, hi = step & _M32, (step >> 32) & _M32
    k = _mix32((base + 0x632BE5AB + lo * 0x9E3779B1) & _M32)
    k = _mix32(k ^ _mix32((hi + 0x7F4A7C15) & _M32))
    j = np.arange(int(b), dtype=np.uint64)
    r = _mix32((np.uint64(k) + j * np.uint64(0x85EBCA6B)) & np.uint64(_M32))
    return (r % np.uint64(T)).astype(np.int64)


def _affine_coords(entries, b, dev):
    """Q17 source coordinates (SX, SY), int64 [b, 28, 28], of every output
    pixel under one table row per image."""
    e = entries.to(device=dev, dtype=torch.int64).view(b, 6, 1, 1)
    u = 2 * torch.arange(_SIDE, device=dev, dtype=torch.int64) - (_SIDE - 1)
    uc, ur = u.view(1, 1, _SIDE), u.view(1, _SIDE, 1)
    half = (_SIDE - 1) * AUG_ONE
    SX = half + e[:, 0] * uc + e[:, 1] * ur + 2 * e[:, 4]
    SY = half + e[:, 2] * uc + e[:, 3] * ur + 2 * e[:, 5]
    return SX, SY


def _bilinear_u8(rows_u8, SX, SY):
    """The part of the warp after the coordinates: x0/y0/fx/fy split of the
    Q17 positions, four predicated taps (background 0), 8-bit weights,
    round to nearest.  Shared by affine_warp_u8 and elastic_warp_u8."""
    b = rows_u8.shape[0]
    x0, y0 = SX >> 17, SY >> 17  # arithmetic shift = floor
    fx, fy = (SX >> 9) & 255, (SY >> 9) & 255
    src = rows_u8.reshape(b, _SIDE * _SIDE).long()

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < _SIDE) & (yy >= 0) & (yy < _SIDE)
        flat = yy.clamp(0, _SIDE - 1) * _SIDE + xx.clamp(0, _SIDE - 1)
        v = src.gather(1, flat.view(b, -1)).view(b, _SIDE, _SIDE)
        return torch.where(ok, v, torch.zeros_like(v))

    top = tap(y0, x0) * (256 - fx) + tap(y0, x0 + 1) * fx
    bot = tap(y0 + 1, x0) * (256 - fx) + tap(y0 + 1, x0 + 1) * fx
    v = (top * (256 - fy) + bot * fy + 32768) >> 16
    return v.to(torch.uint8).view(b, _SIDE * _SIDE)


def affine_warp_u8(rows_u8, entries):
    """Integer bilinear warp of uint8 images.  rows_u8: [b, 784] uint8,
    entries: [b, 6] integer (one table row per image) -> uint8 [b, 784].
    Defined for entries within the builder's bounds (int64 here; the kernel's
    int32 arithmetic agrees there)."""
    SX, SY = _affine_coords(entries, rows_u8.shape[0], rows_u8.device)
    return _bilinear_u8(rows_u8, SX, SY)


# -- elastic distortion (integer only; csrc/elastic_gather.hip mirrors it) ---
#
# Simard et al. 2003: per image and axis a field of uniform noise, smoothed
# by a Gaussian, scaled by alpha, added to the source position of every
# output pixel.  Here the noise is int8, the Gaussian a separable integer
# Toeplitz matrix G (taps summing to <= 256, zero outside the image, no
# renormalisation: the field tapers at the border), and both smoothing passes
# are exact integer matrix products, so any summation order gives the same
# bits.  Flat pixel p = r * 28 + c; axis 0 displaces x (columns), 1 y (rows).

ELASTIC_KEY_ADD = 0x3C6EF372    # separates the field key from aug_indices
ELASTIC_NOISE_MUL = 0xB5297A4D  # odd: element index -> hash input stride
ELASTIC_MAX_ALPHA = 64.0        # px; A = rint(256 alpha) <= 16384
ELASTIC_MAX_A = 16384


def elastic_key(seed: int, step: int, j):
    """32-bit field key of batch position(s) j at `step` -> uint64 numpy
    array (values < 2^32) shaped like j.  The (base, step lo, step hi, j)
    chain of aug_indices under another additive constant: independent of the
    table row choice, full 64-bit step, keyed on the batch POSITION."""
    import numpy as np
    step = int(step)
    if step < 0:
        raise ValueError("step must be >= 0")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    base = _mix32((seed & _M32) ^ _mix32(((seed >> 32) + 0x9E3779B9) & _M32))
    lo, hi = step & _M32, (step >> 32) & _M32
    k = _mix32((base + ELASTIC_KEY_ADD + lo * 0x9E3779B1) & _M32)
    k = _mix32(k ^ _mix32((hi + 0x7F4A7C15) & _M32))
    j = np.asarray(j, dtype=np.uint64)
    return _mix32((np.uint64(k) + j * np.uint64(0x85EBCA6B)) & np.uint64(_M32))


def elastic_noise(keys):
    """int8-valued noise n[a][p] = (mix32(key + (a*784 + p) * C) >> 24) - 128
    in [-128, 127] -> int64 numpy [b, 2, 28, 28] for uint64 keys [b]."""
    import numpy as np
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 1)
    e = np.arange(2 * _SIDE * _SIDE, dtype=np.uint64).reshape(1, -1)
    m = _mix32((keys + e * np.uint64(ELASTIC_NOISE_MUL)) & np.uint64(_M32))
    n = (m >> np.uint64(24)).astype(np.int64) - 128
    return n.reshape(-1, 2, _SIDE, _SIDE)


def check_elastic_taps(taps):
    """The bounds the integer field rests on: 32 non-negative taps, each
    <= 127 (an int8 operand), g[0] + 2 * sum(g[1:]) <= 256, nothing past
    distance 27.  -> int32 numpy [32]."""
    import numpy as np
    g = np.asarray(taps)
    if g.shape != (32,) or g.dtype.kind not in "iu":
        raise ValueError("elastic taps must be 32 integers")
    g = g.astype(np.int64)
    if g.min() < 0 or g.max() > 127 or g[_SIDE:].any() \
            or g[0] + 2 * g[1:].sum() > 256:
        raise ValueError("elastic taps must be in [0, 127], zero past "
                         "distance 27, with weighted sum <= 256")
    return g.astype(np.int32)


def elastic_taps(sigma: float):
    """Integer Gaussian taps -> int32 numpy [32]: R = min(27, ceil(3 sigma)),
    g[d] = rint(256 exp(-d^2 / 2 sigma^2) / Z) for d <= R with Z the sum over
    -R..R, zero beyond; g[0] is then decremented until g[0] + 2 sum_{d>=1}
    g[d] <= 256.  sigma in [1, 16] (below about 0.81 the centre tap would
    pass 127, the int8 operand bound); NaN fails the range check."""
    import numpy as np
    sigma = float(sigma)
    if not (1.0 <= sigma <= 16.0):  # NaN fails both compares
        raise ValueError(f"elastic_taps: sigma={sigma} outside [1, 16]")
    R = min(_SIDE - 1, int(np.ceil(3.0 * sigma)))
    d = np.arange(R + 1, dtype=np.float64)
    w = np.exp(-d * d / (2.0 * sigma * sigma))
    g = np.zeros(32, dtype=np.int64)
    g[:R + 1] = np.rint(256.0 * w / (w[0] + 2.0 * w[1:].sum()))
    while g[0] + 2 * g[1:].sum() > 256:
        g[0] -= 1
    return check_elastic_taps(g)


def elastic_alpha_q(alpha: float) -> int:
    """A = rint(alpha * 256) for alpha in pixels, 0 < alpha <= 64."""
    alpha = float(alpha)
    if not (0.0 < alpha <= ELASTIC_MAX_ALPHA):  # NaN fails both compares
        raise ValueError(f"elastic alpha={alpha} outside (0, 64] pixels")
    return int(round(alpha * 256.0))


def elastic_field(taps, noise):
    """Smoothed integer field of int8-valued noise [..., 28, 28] ->
    (F, T8), both int64 numpy of the same shape.  G[i][k] = g[|i-k|]:

      T  = G . N            |T| <= 256 * 128
      T8 = (T + 128) >> 8   arithmetic shift; in [-128, 127]: the extremes
                            are T = 256 * 127 = 32512 -> 32640 >> 8 = 127
                            and T = -256 * 128 = -32768 -> -32640 >> 8 = -128
      F  = T8 . G^T         |F| <= 128 * 256 = 32768

    F / 32768 is the smoothed field in units of the uniform(-1, 1) noise."""
    import numpy as np
    g = check_elastic_taps(taps).astype(np.int64)
    i = np.arange(_SIDE)
    G = g[np.abs(i[:, None] - i[None, :])]
    n = np.asarray(noise, dtype=np.int64)
    assert n.min() >= -128 and n.max() <= 127
    T8 = (G @ n + 128) >> 8
    assert T8.min() >= -128 and T8.max() <= 127
    F = T8 @ G.T
    assert np.abs(F).max() <= 32768
    return F, T8


def elastic_displacement(taps, alpha_q: int, seed: int, step: int, b: int):
    """dS[j][a][p] = (A * F[a][p]) >> 6 (arithmetic shift; |A * F| <= 2^29)
    for batch positions j < b -> int64 numpy [b, 2, 28, 28]: the
    displacement in the Q17 units of affine_warp_u8's SX / SY.  |dS| <= 2^23
    (64 px), so next to |a| <= 4, |t| <= 64 px (|SX| < 2^25) the sum stays
    far inside int32."""
    import numpy as np
    A = int(alpha_q)
    if not 0 <= A <= ELASTIC_MAX_A:
        raise ValueError(f"elastic alpha_q={A} outside [0, {ELASTIC_MAX_A}]")
    keys = elastic_key(seed, step, np.arange(int(b)))
    F, _ = elastic_field(taps, elastic_noise(keys))
    return (A * F) >> 6


def elastic_warp_u8(rows_u8, entries, dS):
    """affine_warp_u8 with SX + dS[:, 0] and SY + dS[:, 1] per output pixel
    (dS: integer [b, 2, 28, 28]); all-zero dS is affine_warp_u8."""
    b, dev = rows_u8.shape[0], rows_u8.device
    SX, SY = _affine_coords(entries, b, dev)
    d = torch.as_tensor(dS).to(device=dev, dtype=torch.int64)
    return _bilinear_u8(rows_u8, SX + d[:, 0], SY + d[:, 1])


def batch_gather(img_u8, lab_u8, lut, x, y, seed: int, step: int,
                 aug_table=None, elastic=None):
    """x[j] = lut[img_u8[idx[j]]], y[j] = lab_u8[idx[j]] written into the
    caller's buffers (any device; x takes lut's dtype).  With `aug_table`
    (int32 [T, 6]) row j is warped by table entry aug_indices(...)[j]
    between the permutation and the LUT; labels are unchanged.  With
    `elastic` = (taps int [32], A) the warp also adds the displacement field
    of elastic_key(seed, step, j); without a table the affine part is the
    identity."""
    n, b = lab_u8.shape[0], y.shape[0]
    idx = torch.from_numpy(batch_indices(n, b, seed, step)).to(img_u8.device)
    rows = img_u8[idx]
    if aug_table is None and elastic is not None:
        aug_table = torch.tensor([AUG_IDENTITY], dtype=torch.int32)
    if aug_table is not None:
        if aug_table.dim() != 2 or aug_table.shape[1] != 6 \
                or aug_table.shape[0] < 1:
            raise ValueError("aug_table must be [T >= 1, 6]")
        t = torch.from_numpy(aug_indices(aug_table.shape[0], seed, step, b))
        ent = aug_table[t.to(aug_table.device)]
        if elastic is None:
            rows = affine_warp_u8(rows.reshape(b, -1), ent)
        else:
            taps, A = elastic
            taps = torch.as_tensor(taps).cpu().numpy()
            dS = elastic_displacement(taps, A, seed, step, b)
            rows = elastic_warp_u8(rows.reshape(b, -1), ent, dS)
    x.copy_(lut[rows.long()].reshape(x.shape))
    y.copy_(lab_u8[idx].long())
    return x, y


# ---------------------------------------------------------------------------
# Device-side evaluation: sequential chunk gather + accumulated statistics.
# Oracles of csrc/eval_ops.hip (and the CPU / fp32-on-GPU path).
# ---------------------------------------------------------------------------

def range_gather(img_u8, lab_u8, lut, x, y, start: int):
    """Chunk [start, start + B) of the resident set into the caller's
    buffers: a row i < N is lut[img_u8[i]] with its label, a row past N is
    exactly zero with label -1.  start >= N is legal (all padding)."""
    n, b = lab_u8.shape[0], y.shape[0]
    start = int(start)
    if start < 0:
        raise ValueError("start must be >= 0")
    live = max(0, min(b, n - start))
    xf = x.view(b, -1)
    if live:
        xf[:live] = lut[img_u8[start:start + live].long()]
        y[:live] = lab_u8[start:start + live].long()
    if live < b:
        xf[live:] = 0
        y[live:] = -1
    return x, y


def softmax_eval(logits, labels, loss_sum, counts, pred=None,
                 cursor_dev=None):
    """Evaluation statistics of one chunk, ACCUMULATED into the running
    state: loss_sum[0] (fp32) += sum of -log softmax(logits)[label],
    counts (int32 [2 + C*C]) += (live rows, correct rows, confusion[t, p]).
    A row is live iff 0 <= label < C; every other row contributes to
    nothing.  The prediction is the LOWEST index among the maximal logits
    (not torch.argmax, whose tie order is unspecified).  pred (uint8 [B]):
    predicted class, 255 where the row is not live.  cursor_dev (int64 [1])
    advances by B."""
    B, C = logits.shape
    lf = logits.float()
    live = (labels >= 0) & (labels < C)
    mx = lf.max(dim=1, keepdim=True).values
    idx = torch.arange(C, device=logits.device).expand(B, C)
    p = torch.where(lf == mx, idx, torch.full_like(idx, C)).min(dim=1).values
    t = labels.clamp(0, C - 1)
    xl = lf.gather(1, t.view(-1, 1)).squeeze(1)
    row_loss = (lf - mx).exp().sum(dim=1).log() - (xl - mx.squeeze(1))
    loss_sum += row_loss[live].double().sum().to(loss_sum.dtype)
    tl, pl = t[live], p[live]
    counts[0] += int(live.sum())
    counts[1] += int((tl == pl).sum())
    counts[2:] += torch.bincount(tl * C + pl, minlength=C * C).to(counts.dtype)
    if pred is not None:
        pred.copy_(torch.where(live, p, torch.full_like(p, 255)).to(pred.dtype))
    if cursor_dev is not None:
        cursor_dev += B


def plane_reduce(planes, out):
    """The deterministic mode's ordered reduction, in place:
    S = ((p_0 + p_1) + p_2) + ... + p_{P-1} (fp32, planes in index order,
    starting from p_0), then out += S (one fp32 add).  A sequential loop over
    the planes; each step is one elementwise fp32 add, so no reassociation."""
    assert planes.dim() == 2 and planes.shape[0] >= 1
    assert planes.dtype == torch.float32 and out.dtype == torch.float32
    assert out.numel() == planes.shape[1]
    p = planes.detach().cpu()
    s = p[0].clone()
    for i in range(1, p.shape[0]):
        s = s + p[i]
    out += s.to(out.device).view_as(out)
    return out


# ---------------------------------------------------------------------------
# MXFP8 gradient wire (--grad_dtype mxfp8): the bit-exact contract of
# csrc/mxwire.hip (docs/KERNELS.md "MXFP8 gradient wire").  OCP MX: blocks of
# 32 e4m3 codes, one E8M0 scale byte per block; stochastic rounding in integer
# arithmetic on the fp32 bits, nothing ever clipped.
# ---------------------------------------------------------------------------

MX_BLOCK = 32
MX_KEY_ADD = 0x4D58F8E4
MX_NAN_BITS = 0x7FC00000


def mx_shard_blocks(n: int, world: int) -> int:
    """Blocks per shard: ceil(ceil(n / 32) / world) rounded up to a multiple
    of 16, so a shard (32 * sb code bytes, then sb scale bytes) is a multiple
    of 16 B."""
    if n < 1 or not 1 <= world <= 16:
        raise ValueError(f"mx_shard_blocks: n = {n} >= 1, world = {world} in "
                         "1..16")
    nb = -(-n // MX_BLOCK)
    return (-(-nb // world) + 15) // 16 * 16


def mx_key(seed: int, step: int, stage: int, rank: int) -> int:
    """The 32-bit rounding key of one encode: the seed fold and the 64-bit
    step fold of the batch gathers' position keys (MX_KEY_ADD separates the
    users), then the (rank, stage) pair.  Element i draws
    _mix32(key + i * 0x85EBCA6B)."""
    seed &= 0xFFFFFFFFFFFFFFFF
    step &= 0xFFFFFFFFFFFFFFFF
    base = _mix32((seed & _M32) ^ _mix32(((seed >> 32) + 0x9E3779B9) & _M32))
    k = _mix32((base + MX_KEY_ADD + (step & _M32) * 0x9E3779B1) & _M32)
    k = _mix32(k ^ _mix32(((step >> 32) + 0x7F4A7C15) & _M32))
    return _mix32((k + (2 * rank + stage + 1) * 0xC2B2AE35) & _M32)


def mx_encode(x, seed: int, step: int, stage: int, rank: int):
    """Flat fp32 [n] -> (codes uint8 [32 * nb], scales uint8 [nb]), nb =
    ceil(n / 32); elements past n count as zero.

    Scale byte of a block from A = max(bits & 0x7fffffff): 0xFF when A >=
    0x7f800000 (a non-finite element; all codes 0), otherwise
    max(0, (A >> 23) - 8 + ((A & 0x7fffff) > 0x600000)): e = byte - 127 is the
    smallest integer in [-127, 127] with amax * 2^-e <= 448 = 1.75 * 2^8.

    Element: sign, exponent field ef and significand M (24 bits, bit 23 set;
    a subnormal is normalised: M = mant << lz, ef = 1 - lz; zero has M = 0) of
    its fp32 bits.  k = ef - 127 - e is the binade of y = x * 2^-e, sh = 20 +
    max(0, -6 - k) the significand bits below the e4m3 grid (capped at 63),
    T = (M << 32) >> sh in 64 bits: q = T >> 32 grid steps toward zero, and
    one more when the element's random word is below the low 32 bits of T
    (probability remainder / step; exact for sh <= 32, truncated below
    2^-32 of a step beyond, never for sh >= 56).  The magnitude is q * 2^
    (max(k, -6) - 3): code (k + 7) << 3 plus q - 8 for k >= -6 (q = 16 carries
    into the next binade), q itself in the subnormal range; a zero magnitude
    drops the sign."""
    import numpy as np
    if x.dtype != torch.float32 or x.dim() != 1 or x.numel() < 1:
        raise ValueError("mx_encode: x is a non-empty 1-D fp32 tensor")
    n = x.numel()
    nb = -(-n // MX_BLOCK)
    bits = np.zeros(nb * MX_BLOCK, dtype=np.uint32)
    bits[:n] = x.detach().cpu().contiguous().numpy().view(np.uint32)
    mag = (bits & np.uint32(0x7FFFFFFF)).astype(np.int64)
    A = mag.reshape(nb, MX_BLOCK).max(axis=1)
    nonfinite = A >= 0x7F800000
    byte = np.maximum(0, (A >> 23) - 8 + ((A & 0x7FFFFF) > 0x600000))
    e = np.repeat(byte - 127, MX_BLOCK)
    ef = mag >> 23
    mant = mag & 0x7FFFFF
    sub = ef == 0
    lz = 24 - np.frexp(mant.astype(np.float64))[1].astype(np.int64)
    M = np.where(sub, mant << np.where(sub, lz, 0), mant | 0x800000)
    ef = np.where(sub, 1 - lz, ef)
    k = ef - 127 - e
    sh = np.minimum(63, 20 + np.maximum(0, -6 - k))
    T = (M.astype(np.uint64) << np.uint64(32)) >> sh.astype(np.uint64)
    key = mx_key(seed, step, stage, rank)
    i = np.arange(nb * MX_BLOCK, dtype=np.uint64)
    rnd = _mix32((np.uint64(key) + i * np.uint64(0x85EBCA6B))
                 & np.uint64(_M32))
    q = (T >> np.uint64(32)).astype(np.int64) + (
        rnd < (T & np.uint64(_M32))).astype(np.int64)
    code = np.where(k >= -6, ((k + 7) << 3) + q - 8, q)
    code = np.where(q == 0, 0, code | ((bits >> 24) & 0x80))
    code = np.where(np.repeat(nonfinite, MX_BLOCK), 0, code)
    scales = np.where(nonfinite, 0xFF, byte)
    return (torch.from_numpy(code.astype(np.uint8)),
            torch.from_numpy(scales.astype(np.uint8)))


def mx_decode(codes, scales):
    """(codes uint8 [32 * nb], scales uint8 [nb]) -> fp32 [32 * nb], exactly:
    e4m3 value * 2^(byte - 127), computed in float64 (every result is an fp32
    number, subnormal ones included; only a code above 1.875 * 2^7 under byte
    247 leaves the range and gives inf).  Scale byte 0xFF and the e4m3 NaN
    codes (0x7F, 0xFF) give the NaN 0x7fc00000."""
    import numpy as np
    c = codes.detach().cpu().numpy().astype(np.int64)
    s = scales.detach().cpu().numpy().astype(np.int64)
    if c.size != s.size * MX_BLOCK:
        raise ValueError("mx_decode: 32 codes per scale byte")
    E, m = (c >> 3) & 15, c & 7
    v = np.where(E == 0, np.ldexp(m.astype(np.float64), -9),
                 np.ldexp((8 + m).astype(np.float64), E - 10))
    v = np.where(c & 0x80, -v, v)
    sb = np.repeat(s, MX_BLOCK)
    with np.errstate(over="ignore"):
        out = np.ldexp(v, sb - 127).astype(np.float32)
    nan = np.uint32(MX_NAN_BITS).view(np.float32)
    out = np.where((sb == 0xFF) | ((c & 0x7F) == 0x7F), nan, out)
    return torch.from_numpy(out.astype(np.float32))


def mx_to_wire(codes, scales, world: int):
    """The shard layout of one encoded vector: uint8 [world][33 * sb], row w
    = the 32 * sb code bytes of blocks [w * sb, (w + 1) * sb), then their sb
    scale bytes; blocks past nb are zero (codes and scale)."""
    nb = scales.numel()
    sb = (-(-nb // world) + 15) // 16 * 16
    c = torch.zeros(world * sb, MX_BLOCK, dtype=torch.uint8)
    s = torch.zeros(world * sb, dtype=torch.uint8)
    c[:nb] = codes.view(nb, MX_BLOCK)
    s[:nb] = scales
    return torch.cat([c.view(world, sb * MX_BLOCK), s.view(world, sb)], dim=1)


def mx_from_wire(wire):
    """uint8 [W][33 * sb] (or one row [33 * sb]) -> (codes [32 * W * sb],
    scales [W * sb]), the blocks in bucket order."""
    wire = wire.reshape(-1, wire.shape[-1])
    sb = wire.shape[1] // (MX_BLOCK + 1)
    return (wire[:, :sb * MX_BLOCK].reshape(-1).contiguous(),
            wire[:, sb * MX_BLOCK:].reshape(-1).contiguous())


def mx_reduce(payloads, seed: int, step: int, owner: int):
    """The owner's half of the exchange: payloads uint8 [W][33 * sb], row r =
    rank r's encoding of the owner's shard.  Decodes every row, adds in fp32
    in rank order (row 0, then + row 1, ...), and re-encodes the sum with
    stage 1 and rank = owner (element indices local to the shard) -> uint8
    [33 * sb]."""
    payloads = payloads.reshape(-1, payloads.shape[-1])
    acc = None
    for row in payloads:
        v = mx_decode(*mx_from_wire(row))
        acc = v if acc is None else acc + v
    return mx_to_wire(*mx_encode(acc, seed, step, 1, owner), 1)[0]
