"""Autograd wiring for the fused primitives, dispatching CPU-ref vs HIP ext.

Dispatch rule: CUDA tensors -> the in-tree HIP extension (fails loudly if the
.so is missing on a GPU box — _C.ext()); CPU tensors -> ops/cpu_ref.py fp32
reference.  Both paths share autograd semantics so the engine/ and models/
code is device-agnostic.

Mixed precision: parameters are fp32 masters; on GPU the model holds bf16
shadow copies used for compute (passed as the non-differentiable `w_comp` /
`b_comp` args).  Weight gradients are always produced in fp32 so they can
accumulate straight into the flat fp32 all-reduce bucket
(parallel/sync.py).
"""

from __future__ import annotations

import torch

from .. import _C
from . import cpu_ref


def _use_hip(t: torch.Tensor) -> bool:
    # the HIP kernels are the bf16 compute path (bf16 operands, fp32
    # epilogues); fp32-on-GPU routes to the torch reference ops (MIOpen /
    # rocBLAS) — a numerics-debug mode, never the bench path
    return t.is_cuda and t.dtype == torch.bfloat16


class ConvPoolFn(torch.autograd.Function):
    """Fused conv5x5-SAME + bias + ReLU + maxpool2x2s2 (mnist.py:107-127).

    GPU direct-grad mode: when dw_out/db_out (fp32 views into the flat
    all-reduce bucket, pre-zeroed each step) are passed, the backward
    kernels accumulate straight into them and None is returned to autograd
    for w/b — no per-param zeros() or AccumulateGrad adds on the hot path.
    """

    @staticmethod
    def forward(ctx, x, w, b, w_comp, b_comp, need_dx: bool,
                dw_out, db_out, w_t):
        if _use_hip(x):
            y, amax = _C.ext().conv_pool_fwd(x, w_comp, b_comp, w_t)
        else:
            y, amax = cpu_ref.conv_pool_fwd(x, w_comp, b_comp)
        ctx.save_for_backward(x, w_comp, y, amax)
        ctx.need_dx = need_dx
        ctx.outs = (dw_out, db_out) if (dw_out is not None and _use_hip(x)) else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w_comp, y, amax = ctx.saved_tensors
        if _use_hip(dy):
            if ctx.outs is not None:
                dw_out, db_out = ctx.outs
                dx = _C.ext().conv_pool_bwd_into(
                    dy.contiguous(), x, w_comp, y, amax, ctx.need_dx,
                    dw_out, db_out)
                dw = db = None
            else:
                dx, dw, db = _C.ext().conv_pool_bwd(
                    dy.contiguous(), x, w_comp, y, amax, ctx.need_dx)
        else:
            dx, dw, db = cpu_ref.conv_pool_bwd(dy, x, w_comp, y, amax)
        if not ctx.need_dx:
            dx = None
        return dx, dw, db, None, None, None, None, None, None


def conv_pool(x, w, b, w_comp=None, b_comp=None, need_dx=True,
              dw_out=None, db_out=None, w_t=None):
    return ConvPoolFn.apply(x, w, b, w_comp if w_comp is not None else w,
                            b_comp if b_comp is not None else b, need_dx,
                            dw_out, db_out, w_t)


class LinearActFn(torch.autograd.Function):
    """x @ W + b [+ReLU] [+TF-dropout(1-p_keep)] (mnist.py:136-145).

    Dropout is folded into the epilogue; the backward recovers BOTH the relu
    and the dropout mask from sign(y): dropped or relu-clipped positions have
    y == 0, kept positions are scaled by 1/p_keep.
    """

    @staticmethod
    def forward(ctx, x, w, b, w_comp, b_comp, relu: bool, p_keep: float,
                seed: int, offset: int, dw_out, db_out, offset_dev, w_t):
        if _use_hip(x):
            if offset_dev is not None and p_keep < 1.0:
                y = _C.ext().linear_act_fwd_dev(x, w_comp, b_comp, relu,
                                                p_keep, seed, offset_dev,
                                                wT=w_t)
            else:
                y = _C.ext().linear_act_fwd(x, w_comp, b_comp, relu, p_keep,
                                            seed, offset, wT=w_t)
        else:
            y = cpu_ref.linear_fwd(x, w_comp, b_comp, relu)
            if p_keep < 1.0:
                gen = torch.Generator(device="cpu")
                gen.manual_seed((seed * 0x9E3779B97F4A7C15 + offset) % (2**63))
                mask = (torch.rand(y.shape, generator=gen) < p_keep)
                y = y * mask.to(device=y.device, dtype=y.dtype) / p_keep
        ctx.save_for_backward(x, w_comp, y)
        ctx.relu = relu
        ctx.p_keep = p_keep
        ctx.outs = (dw_out, db_out) if (dw_out is not None and _use_hip(x)) else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w_comp, y = ctx.saved_tensors
        relu, p_keep = ctx.relu, ctx.p_keep
        if _use_hip(dy):
            if ctx.outs is not None:
                dw_out, db_out = ctx.outs
                dx = _C.ext().linear_act_bwd_into(
                    dy.contiguous(), x, w_comp, y, relu, p_keep,
                    ctx.needs_input_grad[0], dw_out, db_out)
                dw = db = None
            else:
                dx, dw, db = _C.ext().linear_act_bwd(
                    dy.contiguous(), x, w_comp, y, relu, p_keep,
                    ctx.needs_input_grad[0])
        else:
            dyf = dy.float()
            if relu or p_keep < 1.0:
                dyf = dyf * (y > 0).float()
                if p_keep < 1.0:
                    dyf = dyf / p_keep
            dx = (dyf @ w_comp.float().t()).to(x.dtype)
            dw = x.float().t() @ dyf
            db = dyf.sum(dim=0)
        if not ctx.needs_input_grad[0]:
            dx = None
        return (dx, dw, db, None, None, None, None, None, None, None, None,
                None, None)


def linear_act(x, w, b, w_comp=None, b_comp=None, relu=False, p_keep=1.0,
               seed=0, offset=0, dw_out=None, db_out=None, offset_dev=None,
               w_t=None):
    return LinearActFn.apply(x, w, b, w_comp if w_comp is not None else w,
                             b_comp if b_comp is not None else b, relu,
                             float(p_keep), int(seed), int(offset),
                             dw_out, db_out, offset_dev, w_t)


class SoftmaxXentFn(torch.autograd.Function):
    """Fused mean sparse-softmax-CE + top-1-correct count (mnist.py:149-164).

    Forward also produces dlogits = (softmax - onehot)/B so backward is a
    saved-tensor multiply — one fused GPU kernel total.
    Returns (loss, correct_count); correct_count is non-differentiable.
    """

    @staticmethod
    def forward(ctx, logits, labels):
        if _use_hip(logits):
            loss, correct, dl = _C.ext().softmax_xent_fwd(logits, labels)
        else:
            loss, correct, dl = cpu_ref.softmax_xent_fwd(logits, labels)
        ctx.save_for_backward(dl)
        ctx.mark_non_differentiable(correct)
        return loss, correct

    @staticmethod
    def backward(ctx, dloss, _dcorrect):
        (dl,) = ctx.saved_tensors
        return (dl * dloss).to(dl.dtype), None


def softmax_xent(logits, labels):
    return SoftmaxXentFn.apply(logits, labels)


def grad_mask(grad: torch.Tensor, keep: float, seed: int, step: int,
              rank: int, step_dev=None, base: int = 0):
    """Per-rank PRE-AGGREGATION drop-connect: in-place Bernoulli(keep) mask
    of this rank's local gradient BEFORE the all-reduce, seeded by
    (seed, step, rank) so every worker's mask is distinct — the reference's
    estimator (distributed_train.py:194-203: masks applied per worker, then
    averaged).  Mask, NO rescale (:414-416)."""
    if grad.is_cuda:
        _C.ext().grad_mask(grad, float(keep), int(seed), int(step),
                           int(rank), base=int(base), step_dev=step_dev)
    else:
        gen = torch.Generator(device="cpu")
        gen.manual_seed(((seed ^ 0x9D5AD0C5) * 0x9E3779B97F4A7C15
                         + (step << 20) + rank + 1) % (2**63))
        mask = (torch.rand(grad.shape, generator=gen) < keep).float()
        grad.mul_(mask.to(grad.device))


_IDENTITY_TABLES: dict = {}


def _identity_table(device) -> torch.Tensor:
    """One-row identity transform table, uploaded once per device (a call
    under hipGraph capture must not copy from the host)."""
    if device not in _IDENTITY_TABLES:
        _IDENTITY_TABLES[device] = torch.tensor(
            [cpu_ref.AUG_IDENTITY], dtype=torch.int32, device=device)
    return _IDENTITY_TABLES[device]


def batch_gather(img_u8: torch.Tensor, lab_u8: torch.Tensor,
                 lut: torch.Tensor, x: torch.Tensor, y: torch.Tensor,
                 seed: int, step: int | None = None, step_dev=None,
                 aug_table: torch.Tensor | None = None, elastic=None):
    """Build the batch at `step` from the resident uint8 training set into
    the caller's buffers: x[j] = lut[img[perm(...)]] ([B,28,28,1], lut's
    dtype), y[j] = labels ([B] int64).  The sample order is a pure function
    of (seed, step) — ops/cpu_ref.py::batch_indices.  Exactly one of `step`
    (host int) / `step_dev` (device int64, hipGraph-capturable on the HIP
    path) is given.  With `aug_table` (int32 [T,6], ops/cpu_ref.py::
    augment_table) image j is warped by table row aug_indices(seed, step, j)
    before the LUT (batch_gather_aug_kernel on the HIP path); without it the
    plain kernel runs.  With `elastic` = (taps int32 [32], alpha_q) the
    displacement field of ops/cpu_ref.py::elastic_displacement is added to
    the warp (batch_gather_elastic_kernel on the HIP path), over a one-row
    identity table when no `aug_table` is given (cached per device after the
    first call; pass a table when the first call is captured)."""
    if (step is None) == (step_dev is None):
        raise ValueError("batch_gather: pass exactly one of step / step_dev")
    if y.shape[0] > lab_u8.shape[0]:
        raise ValueError(f"batch size {y.shape[0]} exceeds the "
                         f"{lab_u8.shape[0]} examples of this rank")
    if aug_table is not None and (
            aug_table.dtype != torch.int32 or aug_table.dim() != 2
            or aug_table.shape[1] != 6 or aug_table.shape[0] < 1):
        raise ValueError("batch_gather: aug_table must be int32 [T >= 1, 6]")
    if elastic is not None:
        taps, alpha_q = elastic
        if taps.dtype != torch.int32 or tuple(taps.shape) != (32,):
            raise ValueError("batch_gather: elastic taps must be int32 [32]")
        if not 0 <= int(alpha_q) <= cpu_ref.ELASTIC_MAX_A:
            raise ValueError(f"batch_gather: elastic alpha_q {alpha_q} "
                             f"outside [0, {cpu_ref.ELASTIC_MAX_A}]")
        if aug_table is None:
            aug_table = _identity_table(x.device)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if _use_hip(x):
        if seed >= 1 << 63:
            seed -= 1 << 64  # int64 carrier of the same 64 bits
        if elastic is not None:
            _C.ext().batch_gather_elastic(
                img_u8, lab_u8, lut, aug_table, taps, int(alpha_q), x, y,
                seed, 0 if step is None else int(step), step_dev=step_dev)
        elif aug_table is None:
            _C.ext().batch_gather(img_u8, lab_u8, lut, x, y, seed,
                                  0 if step is None else int(step),
                                  step_dev=step_dev)
        else:
            _C.ext().batch_gather_aug(img_u8, lab_u8, lut, aug_table, x, y,
                                      seed, 0 if step is None else int(step),
                                      step_dev=step_dev)
    else:
        if step is None:
            step = int(step_dev.item())  # reference path: host sync is fine
        cpu_ref.batch_gather(img_u8, lab_u8, lut, x, y, seed, int(step),
                             aug_table=aug_table, elastic=elastic)
    return x, y


def range_gather(img_u8: torch.Tensor, lab_u8: torch.Tensor,
                 lut: torch.Tensor, x: torch.Tensor, y: torch.Tensor,
                 start: int | None = None, start_dev=None):
    """Sequential chunk [start, start + B) of the resident uint8 set into
    the caller's buffers, tail included: rows past N are zero-filled with
    label -1 (ops/cpu_ref.py::range_gather).  Exactly one of `start` (host
    int) / `start_dev` (device int64, hipGraph-capturable on the HIP path)
    is given.  Unlike batch_gather, B > N and start >= N are legal."""
    if (start is None) == (start_dev is None):
        raise ValueError("range_gather: pass exactly one of start / start_dev")
    if _use_hip(x):
        _C.ext().range_gather(img_u8, lab_u8, lut, x, y,
                              0 if start is None else int(start),
                              start_dev=start_dev)
    else:
        if start is None:
            start = int(start_dev.item())  # reference path: host sync is fine
        cpu_ref.range_gather(img_u8, lab_u8, lut, x, y, int(start))
    return x, y


def softmax_eval(logits: torch.Tensor, labels: torch.Tensor,
                 loss_sum: torch.Tensor, counts: torch.Tensor, pred=None,
                 cursor_dev=None):
    """Accumulate one chunk's evaluation statistics into the running state
    (loss_sum fp32 [1], counts int32 [2 + C*C]: live rows, correct rows,
    confusion[true, predicted]); rows whose label lies outside [0, C)
    contribute to nothing.  Optional pred (uint8 [B], 255 = not live) and
    cursor_dev (int64 [1], advanced by B).  No autograd: this is the
    evaluation kernel, it produces no dlogits."""
    if _use_hip(logits):
        _C.ext().softmax_eval(logits, labels, loss_sum, counts, pred=pred,
                              cursor_dev=cursor_dev)
    else:
        cpu_ref.softmax_eval(logits, labels, loss_sum, counts, pred=pred,
                             cursor_dev=cursor_dev)


def grad_norm(flat: torch.Tensor, offsets, numels, grad_scale: float,
              clip: float, stats=None, clipped_steps=None):
    """Per-tensor and global L2 norms of the flat fp32 gradient `flat` (the
    SUM over contributors, grad_scale = 1 / contributors) and the
    clip_grad_norm_ coefficient -> `stats` (fp32 [2 + segments]: norm,
    min(1, clip / (norm + 1e-6)), then one norm per (offset, numel) segment;
    ops/cpu_ref.py::grad_norm).  `stats` is written in place when given;
    `clipped_steps` (int64 [1], optional) counts the calls whose coefficient
    is below 1.  On the GPU one grad_norm_kernel launch: device-resident,
    hipGraph-capturable (after a first call outside capture), no float
    atomics, so equal inputs give equal bits."""
    offsets, numels = [int(o) for o in offsets], [int(m) for m in numels]
    if stats is None:
        stats = torch.empty(2 + len(offsets), dtype=torch.float32,
                            device=flat.device)
    if flat.is_cuda:
        if clipped_steps is None:
            clipped_steps = torch.zeros(1, dtype=torch.int64,
                                        device=flat.device)
        _C.ext().grad_norm(flat, offsets, numels, float(grad_scale),
                           float(clip), stats, clipped_steps)
    else:
        stats.copy_(cpu_ref.grad_norm(flat, offsets, numels, grad_scale,
                                      clip))
        if clipped_steps is not None and float(stats[1]) < 1.0:
            clipped_steps += 1
    return stats


def topk_compress(g: torch.Tensor, r: torch.Tensor, offsets, numels, ks,
                  payload=None, dense: bool = True):
    """Top-k sparsification with error feedback of the flat fp32 bucket `g`
    against the residual `r` (ops/cpu_ref.py::topk_compress is the contract):
    r += g, the ks[t] largest magnitudes of every (offset, numel) segment
    leave r for `payload` (int32 [2][sum(ks)], written in place when given).
    `g` is rewritten IN PLACE: the selected values and zeros elsewhere, or
    all zeros with dense=False (the multi-rank exchange scatters every rank's
    pairs into it).  Returns (payload, g).  On the GPU the five launches of
    csrc/topk.hip: device-resident, hipGraph-capturable (after a first call
    outside capture), integer atomics only, so equal inputs give equal
    bits."""
    offsets, numels = [int(o) for o in offsets], [int(m) for m in numels]
    ks = [int(k) for k in ks]
    if payload is None:
        payload = torch.empty(2, sum(ks), dtype=torch.int32, device=g.device)
    if g.is_cuda:
        _C.ext().topk_compress(g, r, offsets, numels, ks, payload,
                               dense=bool(dense))
    else:
        p, d = cpu_ref.topk_compress(g, r, offsets, numels, ks)
        payload.copy_(p)
        if dense:
            g.copy_(d)
        else:
            g.zero_()
    return payload, g


def topk_scatter(payloads: torch.Tensor, n: int, out=None):
    """Dense fp32 bucket [n] of the ranks' payloads (int32 [W][2][K]): zeros,
    then every rank's pairs added in rank order (ops/cpu_ref.py::
    topk_scatter).  `out`, when given, is the bucket to fill and must hold
    zeros.  On the GPU one topk_scatter_kernel launch per rank on the current
    stream, which fixes the order of the sums."""
    payloads = payloads.reshape(-1, 2, payloads.shape[-1])
    if out is None:
        out = torch.zeros(n, dtype=torch.float32, device=payloads.device)
    if out.numel() != n:
        raise ValueError(f"topk_scatter: out holds {out.numel()} values, "
                         f"not {n}")
    if payloads.is_cuda:
        for w in range(payloads.shape[0]):
            _C.ext().topk_scatter(payloads[w], out, assign=(w == 0))
    else:
        out.copy_(cpu_ref.topk_scatter(payloads, n))
    return out


def mx_encode(x: torch.Tensor, seed: int, step: int, stage: int, rank: int,
              world: int = 1, out=None, keep=None, step_dev=None):
    """MXFP8 wire of the flat fp32 vector `x` (ops/cpu_ref.py::mx_encode is
    the contract): uint8 [world][33 * sb] in the shard layout of
    cpu_ref.mx_to_wire, 32 e4m3 codes per E8M0 scale byte, rounded
    stochastically under the key (seed, step, stage, rank, element index).
    `out` is written in place when given; `keep` (fp32 [n], optional) receives
    a copy of x.  On the GPU one mx_encode_kernel launch, hipGraph-capturable;
    `step_dev` (int64 [1]) then replaces `step`, read on the device."""
    n = x.numel()
    sb = cpu_ref.mx_shard_blocks(n, world)
    if out is None:
        out = torch.empty(world, 33 * sb, dtype=torch.uint8, device=x.device)
    if x.is_cuda:
        _C.ext().mx_encode(x, out, int(world), int(seed), int(step),
                           int(stage), int(rank), keep=keep,
                           step_dev=step_dev)
    else:
        if step_dev is not None:
            step = int(step_dev.item())
        out.copy_(cpu_ref.mx_to_wire(
            *cpu_ref.mx_encode(x, seed, step, stage, rank), world))
        if keep is not None:
            keep.copy_(x)
    return out


def mx_reduce(rows: torch.Tensor, seed: int, step: int, owner: int, out=None,
              step_dev=None):
    """One shard of the MXFP8 exchange: `rows` uint8 [W][33 * sb] (row r =
    rank r's encoding of this shard) decoded, added in fp32 in rank order and
    re-encoded with stage 1 and rank = owner -> uint8 [33 * sb]
    (ops/cpu_ref.py::mx_reduce).  On the GPU one mx_reduce_kernel launch; the
    fp32 sum stays in registers."""
    rows = rows.reshape(-1, rows.shape[-1])
    if out is None:
        out = torch.empty(rows.shape[1], dtype=torch.uint8, device=rows.device)
    if rows.is_cuda:
        _C.ext().mx_reduce(rows, out, int(seed), int(step), int(owner),
                           step_dev=step_dev)
    else:
        if step_dev is not None:
            step = int(step_dev.item())
        out.copy_(cpu_ref.mx_reduce(rows, seed, step, owner))
    return out


def mx_decode(wire: torch.Tensor, n: int, out=None):
    """fp32 [n] of an MXFP8 wire uint8 [W][33 * sb], exactly
    (ops/cpu_ref.py::mx_decode); `out` is written in place when given and
    nothing is written past n.  On the GPU one mx_decode_kernel launch."""
    wire = wire.reshape(-1, wire.shape[-1])
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=wire.device)
    if out.numel() != n or wire.shape[1] != 33 * cpu_ref.mx_shard_blocks(
            n, wire.shape[0]):
        raise ValueError(f"mx_decode: wire {tuple(wire.shape)} / out "
                         f"{out.numel()} do not hold {n} values")
    if wire.is_cuda:
        _C.ext().mx_decode(wire, wire.shape[0], out)
    else:
        out.copy_(cpu_ref.mx_decode(*cpu_ref.mx_from_wire(wire))[:n])
    return out


class LowrankState:
    """--grad_lowrank R: the plan and the persistent buffers of PowerSGD
    compression on one flat bucket of `n` values (ops/cpu_ref.py::lowrank_step
    is the contract).  resid [n]: the error-feedback residual, zero over the
    dense tensors; between lowrank_p and lowrank_expand it holds M = G + E.
    q: the warm-start factors [Q_0 | Q_1 | ..], Q [cols][R].  wire: [P_0 |
    P_1 | .. | dense tensors], P [rows][R]; the dense tail exists only with
    `pack` (more than one rank), where wire and q are the two all-reduce
    payloads.  qr: this rank's Q_r; without `pack` it IS q."""

    def __init__(self, shapes, offsets, n: int, R: int, seed: int, device,
                 pack: bool):
        self.R, self.n, self.pack = int(R), int(n), bool(pack)
        self.plan = cpu_ref.lowrank_plan(shapes, offsets, R)
        if not self.plan:
            raise ValueError("--grad_lowrank: no tensor of this model can be "
                             "compressed")
        self.offsets = [p[1] for p in self.plan]
        self.rows = [p[2] for p in self.plan]
        self.cols = [p[3] for p in self.plan]
        # the dense gaps of the bucket, in order: (bucket offset, length)
        self.gaps, at = [], 0
        for o, r, c in zip(self.offsets, self.rows, self.cols):
            if o > at:
                self.gaps.append((at, o - at))
            at = o + r * c
        if n > at:
            self.gaps.append((at, n - at))
        self.p_floats = self.R * sum(self.rows)
        self.q_floats = self.R * sum(self.cols)
        self.dense_floats = sum(m for _, m in self.gaps)
        self.resid = torch.zeros(n, dtype=torch.float32, device=device)
        self.q = cpu_ref.lowrank_q_init(self.plan, R, seed).to(device)
        self.qr = torch.zeros_like(self.q) if pack else self.q
        self.wire = torch.zeros(
            self.p_floats + (self.dense_floats if pack else 0),
            dtype=torch.float32, device=device)

    def views(self, flat, t, width=None):
        """tensor t's matrix inside a bucket-shaped buffer (width None), or
        its [.][R] factor inside wire (width = rows) / q (width = cols)"""
        if width is None:
            o, r, c = self.offsets[t], self.rows[t], self.cols[t]
            return flat[o:o + r * c].view(r, c)
        o = self.R * sum(width[:t])
        return flat[o:o + width[t] * self.R].view(width[t], self.R)


def lowrank_p(g: torch.Tensor, st: LowrankState):
    """PowerSGD, first half: on every compressed tensor st.resid becomes M =
    G + E and P = M Q goes into st.wire; with st.pack the dense tensors of
    `g` are copied behind P, so that ONE all-reduce of st.wire sums both.  On
    the GPU lowrank_p_kernel: one pass over G and E, fp32 MFMA."""
    if g.is_cuda:
        _C.ext().lowrank_p(g, st.resid, st.q, st.wire, st.offsets, st.rows,
                           st.cols, st.R, pack=st.pack)
        return
    for t in range(len(st.plan)):
        M = st.views(st.resid, t)
        M += st.views(g, t)
        st.views(st.wire, t, st.rows).copy_(M @ st.views(st.q, t, st.cols))
    at = st.p_floats
    for o, m in st.gaps if st.pack else ():
        st.wire[at:at + m] = g[o:o + m]
        at += m


def lowrank_q(st: LowrankState):
    """PowerSGD, between the two sums over ranks: P in st.wire is
    orthonormalised in place (modified Gram-Schmidt), then st.qr = M^T P.  On
    the GPU lowrank_orth_kernel + lowrank_q_kernel, fixed summation orders."""
    if st.wire.is_cuda:
        _C.ext().lowrank_q(st.resid, st.wire, st.qr, st.offsets, st.rows,
                           st.cols, st.R)
        return
    for t in range(len(st.plan)):
        P = st.views(st.wire, t, st.rows)
        P.copy_(cpu_ref.lowrank_orth(P))
        st.views(st.qr, t, st.cols).copy_(st.views(st.resid, t).t() @ P)


def lowrank_expand(g: torch.Tensor, st: LowrankState):
    """PowerSGD, last part: on every compressed tensor g = P Q_S^T (st.q, the
    sum over ranks) and st.resid = M - P Q_r^T (st.qr); with one rank the
    product is formed once and serves both.  With st.pack the summed dense
    tensors return from st.wire into g.  On the GPU lowrank_expand_kernel."""
    if g.is_cuda:
        _C.ext().lowrank_expand(g, st.resid, st.wire, st.qr, st.q, st.offsets,
                                st.rows, st.cols, st.R, pack=st.pack)
        return
    for t in range(len(st.plan)):
        P = st.views(st.wire, t, st.rows)
        M = st.views(st.resid, t)
        own = P @ st.views(st.qr, t, st.cols).t()
        st.views(g, t).copy_(
            P @ st.views(st.q, t, st.cols).t() if st.pack else own)
        M -= own
    at = st.p_floats
    for o, m in st.gaps if st.pack else ():
        g[o:o + m] = st.wire[at:at + m]
        at += m


def lars_norm(master: torch.Tensor, flat: torch.Tensor, offsets, numels,
              adapt_mask: int, grad_scale: float, eta: float, wd: float,
              clip: float = 0.0, lars_tab=None, lars_stats=None,
              clip_stats=None, clipped_steps=None):
    """LARS trust ratios of the flat fp32 `master` and the flat fp32 gradient
    `flat` -> (`lars_tab` fp32 [32], `lars_stats` fp32 [3 * segments]), both
    written in place when given (ops/cpu_ref.py::lars_norm).  clip > 0 also
    fills `clip_stats` / counts in `clipped_steps` exactly as grad_norm()
    does, so the caller needs no grad_norm() call.  On the GPU one
    lars_norm_kernel launch: device-resident, hipGraph-capturable (after a
    first call outside capture), no float atomics."""
    offsets, numels = [int(o) for o in offsets], [int(m) for m in numels]
    dev = flat.device
    if lars_tab is None:
        lars_tab = torch.zeros(32, dtype=torch.float32, device=dev)
    if lars_stats is None:
        lars_stats = torch.empty(3 * len(offsets), dtype=torch.float32,
                                 device=dev)
    if clip > 0 and clip_stats is None:
        clip_stats = torch.empty(2 + len(offsets), dtype=torch.float32,
                                 device=dev)
    if flat.is_cuda:
        if clip > 0 and clipped_steps is None:
            clipped_steps = torch.zeros(1, dtype=torch.int64, device=dev)
        _C.ext().lars_norm(master, flat, offsets, numels, int(adapt_mask),
                           float(grad_scale), float(eta), float(wd),
                           float(clip), lars_tab, lars_stats,
                           clip_stats=clip_stats if clip > 0 else None,
                           clipped_steps=clipped_steps if clip > 0 else None)
    else:
        tab, stats, cs = cpu_ref.lars_norm(master, flat, offsets, numels,
                                           adapt_mask, grad_scale, eta, wd,
                                           clip)
        lars_tab.copy_(tab)
        lars_stats.copy_(stats)
        if cs is not None:
            clip_stats.copy_(cs)
            if clipped_steps is not None and float(cs[1]) < 1.0:
                clipped_steps += 1
    return lars_tab, lars_stats


def sgd_step(master: torch.Tensor, grad: torch.Tensor, lr: float,
             grad_scale: float = 1.0, drop_connect_keep=None,
             seed: int = 0, offset: int = 0, shadow=None,
             momentum=None, mu: float = 0.0, ema=None,
             ema_decay: float = 0.0, clip_coef=None, lars_tab=None,
             offsets=None, numels=None):
    """Fused flat SGD apply: master -= lr*scale*(grad [* bernoulli(keep)]).

    `lars_tab` (with `offsets`, `numels`; not with `clip_coef`): lars_norm()'s
    table on master's device.  Tensor t does g = tab[2t]*g, the drop-connect
    mask, the unmasked decay g += tab[2t + 1]*w, then momentum.

    `clip_coef` (optional one-element fp32 tensor on master's device,
    grad_norm()'s stats[1:2]) multiplies the gradient first, before the
    drop-connect mask and before momentum; it is read on the device.

    Optionally refreshes the bf16 `shadow` copy (one kernel on GPU).
    Reference semantics: GradientDescentOptimizer + drop_connect mask with NO
    rescale (distributed_train.py:176,414-416).
    `ema` (optional fp32, master's layout) is moved towards the new master
    in the same pass: e -= (1 - d_k)*(e - w), d_k = min(ema_decay,
    (1 + k)/(10 + k)), k = offset + 1 (ops/cpu_ref.py::sgd_step).
    """
    if ema is not None and not 0.0 <= ema_decay < 1.0:
        raise ValueError(f"ema_decay must lie in [0, 1), got {ema_decay}")
    lars = {}
    if lars_tab is not None:
        lars = dict(lars_tab=lars_tab, offsets=[int(o) for o in offsets],
                    numels=[int(m) for m in numels])
    if master.is_cuda:
        _C.ext().sgd_step(master, grad,
                          shadow if shadow is not None else master,
                          shadow is not None, float(lr), float(grad_scale),
                          -1.0 if drop_connect_keep is None else float(drop_connect_keep),
                          int(seed), int(offset),
                          momentum=momentum, mu=float(mu), ema=ema,
                          ema_decay=float(ema_decay), clip_coef=clip_coef,
                          **lars)
    else:
        gen = None
        if drop_connect_keep is not None:
            gen = torch.Generator(device="cpu")
            gen.manual_seed((seed * 0x9E3779B97F4A7C15 + offset) % (2**63))
        cpu_ref.sgd_step(master, grad, lr, grad_scale,
                         drop_connect_keep, gen, shadow,
                         momentum=momentum, mu=mu, ema=ema,
                         ema_decay=ema_decay, offset=offset,
                         clip_coef=clip_coef, **lars)


def _cpu_gen(drop_connect_keep, seed, offset):
    if drop_connect_keep is None:
        return None
    gen = torch.Generator(device="cpu")
    gen.manual_seed((seed * 0x9E3779B97F4A7C15 + offset) % (2**63))
    return gen


def adam_step(master: torch.Tensor, grad: torch.Tensor, m: torch.Tensor,
              v: torch.Tensor, lr: float, grad_scale: float = 1.0,
              beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
              wd: float = 0.0, offsets=None, numels=None, adapt_mask: int = 0,
              drop_connect_keep=None, seed: int = 0, offset: int = 0,
              shadow=None, ema=None, ema_decay: float = 0.0, clip_coef=None,
              lr_scale_dev=None, offset_dev=None, zero_grad: bool = False):
    """Fused flat Adam / AdamW update k = offset + 1 (ops/cpu_ref.py::
    adam_step): the moments `m`, `v` and `master` in place, decoupled decay
    `wd` on the tensors (offsets, numels) whose bit is set in `adapt_mask`,
    then the moving average and the bf16 shadow as sgd_step().  `grad` is the
    SUM over contributors, grad_scale = 1 / contributors; `clip_coef`
    multiplies it first.  On the GPU one adam_step_kernel launch; with
    `lr_scale_dev` / `offset_dev` (fp32 lr * grad_scale and int64 offset on
    the device) it is hipGraph-capturable, and `zero_grad` clears the bucket
    in the same pass."""
    if ema is not None and not 0.0 <= ema_decay < 1.0:
        raise ValueError(f"ema_decay must lie in [0, 1), got {ema_decay}")
    offsets = [0] if offsets is None else [int(o) for o in offsets]
    numels = [master.numel()] if numels is None else [int(x) for x in numels]
    if master.is_cuda:
        _C.ext().adam_step(
            master, grad, m, v, float(lr), float(grad_scale), float(beta1),
            float(beta2), float(eps), float(wd), offsets, numels,
            int(adapt_mask),
            -1.0 if drop_connect_keep is None else float(drop_connect_keep),
            int(seed), int(offset), shadow=shadow, ema=ema,
            ema_decay=float(ema_decay), clip_coef=clip_coef,
            lr_scale_dev=lr_scale_dev, offset_dev=offset_dev,
            zero_grad=bool(zero_grad))
    else:
        cpu_ref.adam_step(master, grad, m, v, lr, grad_scale, beta1, beta2,
                          eps, wd, offsets, numels, adapt_mask,
                          drop_connect_keep,
                          _cpu_gen(drop_connect_keep, seed, offset),
                          shadow=shadow, ema=ema, ema_decay=ema_decay,
                          offset=offset, clip_coef=clip_coef)
        if zero_grad:
            grad.zero_()
    return master


def lamb_step(master: torch.Tensor, grad: torch.Tensor, m: torch.Tensor,
              v: torch.Tensor, lr: float, grad_scale: float, beta1: float,
              beta2: float, eps: float, wd: float, offsets, numels,
              adapt_mask: int, lamb_tab=None, lamb_stats=None,
              drop_connect_keep=None, seed: int = 0, offset: int = 0,
              shadow=None, ema=None, ema_decay: float = 0.0, clip_coef=None,
              lr_scale_dev=None, offset_dev=None, zero_grad: bool = False):
    """LAMB update k = offset + 1 (You et al. 2019; ops/cpu_ref.py::
    lamb_moments + lamb_apply): Adam's moments, u_t = u + wd_t * w, the trust
    ratio r_t = |w_t| / |u_t| of every tensor in `adapt_mask` (1 elsewhere
    and for a zero norm), w -= lr * r_t * u_t.  `lamb_tab` (fp32 [16], r_t)
    and `lamb_stats` (fp32 [3 * segments]: |w_t|, |u_t|, r_t) are written in
    place when given.  On the GPU two launches and no host round trip:
    lamb_moments_kernel (fixed-order reduction, no float atomics) and
    lamb_apply_kernel; the other arguments as adam_step().  Returns
    (lamb_tab, lamb_stats)."""
    if ema is not None and not 0.0 <= ema_decay < 1.0:
        raise ValueError(f"ema_decay must lie in [0, 1), got {ema_decay}")
    offsets, numels = [int(o) for o in offsets], [int(x) for x in numels]
    dev = master.device
    if lamb_tab is None:
        lamb_tab = torch.ones(16, dtype=torch.float32, device=dev)
    if lamb_stats is None:
        lamb_stats = torch.zeros(3 * len(offsets), dtype=torch.float32,
                                 device=dev)
    hp = (float(beta1), float(beta2), float(eps), float(wd), offsets, numels,
          int(adapt_mask))
    if master.is_cuda:
        ext = _C.ext()
        ext.lamb_moments(
            master, grad, m, v, float(grad_scale), *hp,
            -1.0 if drop_connect_keep is None else float(drop_connect_keep),
            int(seed), int(offset), lamb_tab, lamb_stats,
            clip_coef=clip_coef, offset_dev=offset_dev)
        ext.lamb_apply(master, grad, m, v, float(lr), float(grad_scale), *hp,
                       int(offset), lamb_tab, shadow=shadow, ema=ema,
                       ema_decay=float(ema_decay), lr_scale_dev=lr_scale_dev,
                       offset_dev=offset_dev, zero_grad=bool(zero_grad))
    else:
        tab, stats = cpu_ref.lamb_moments(
            master, grad, m, v, grad_scale, *hp, offset=offset,
            clip_coef=clip_coef, drop_connect_keep=drop_connect_keep,
            gen=_cpu_gen(drop_connect_keep, seed, offset))
        lamb_tab.copy_(tab)
        lamb_stats.copy_(stats)
        cpu_ref.lamb_apply(master, m, v, lamb_tab, lr, grad_scale, *hp,
                           offset=offset, shadow=shadow, ema=ema,
                           ema_decay=ema_decay)
        if zero_grad:
            grad.zero_()
    return lamb_tab, lamb_stats


def muon_orthogonalize(x: torch.Tensor, iters: int = 5, route: str = "auto"):
    """bf16 Newton-Schulz orthogonalisation of one [rows][cols] matrix
    (ops/cpu_ref.py::muon_orthogonalize).  On the GPU `route` picks the
    kernels: "lds" (muon_ns_lds_kernel: cols <= 64, the matrix resident in
    one workgroup's LDS), "tiled" (the Gram / polynomial / apply kernels:
    cols % 64 == 0, rows % 8 == 0) or "auto", the trainer's choice; a route
    the shape does not fit is an error."""
    if x.is_cuda:
        return _C.ext().muon_orthogonalize(x, int(iters), str(route))
    if route not in ("auto", "lds", "tiled"):
        raise ValueError("muon_orthogonalize: route is auto, lds or tiled")
    return cpu_ref.muon_orthogonalize(x, iters)


def muon_step(master: torch.Tensor, grad: torch.Tensor, mom: torch.Tensor,
              lr: float, grad_scale: float, mu: float, wd: float, offsets,
              numels, cols, adapt_mask: int, drop_connect_keep=None,
              seed: int = 0, offset: int = 0, shadow=None, ema=None,
              ema_decay: float = 0.0, clip_coef=None, lr_scale_dev=None,
              offset_dev=None, zero_grad: bool = False, iters: int = 5):
    """Muon update k = offset + 1 (ops/cpu_ref.py::muon_step): Nesterov
    momentum in `mom`; every tensor of `adapt_mask`, viewed as
    [numel / cols[t]][cols[t]], moves along the Newton-Schulz orthogonalisation
    of its update, scaled by 0.2 * sqrt(max(rows, cols)), with decoupled decay
    `wd`; the biases take plain heavy-ball momentum.  On the GPU the kernel
    sequence of csrc/muon.hip (momentum pass, one LDS-resident launch for the
    narrow tensors, four launches per iteration for each tiled one, the update
    pass), device-resident and hipGraph-capturable after a first call outside
    capture; the other arguments as adam_step()."""
    if ema is not None and not 0.0 <= ema_decay < 1.0:
        raise ValueError(f"ema_decay must lie in [0, 1), got {ema_decay}")
    offsets, numels = [int(o) for o in offsets], [int(x) for x in numels]
    cols = [int(c) for c in cols]
    if master.is_cuda:
        _C.ext().muon_step(
            master, grad, mom, float(lr), float(grad_scale), float(mu),
            float(wd), offsets, numels, cols, int(adapt_mask),
            -1.0 if drop_connect_keep is None else float(drop_connect_keep),
            int(seed), int(offset), iters=int(iters), shadow=shadow, ema=ema,
            ema_decay=float(ema_decay), clip_coef=clip_coef,
            lr_scale_dev=lr_scale_dev, offset_dev=offset_dev,
            zero_grad=bool(zero_grad))
    else:
        cpu_ref.muon_step(master, grad, mom, lr, grad_scale, mu, wd, offsets,
                          numels, cols, adapt_mask, drop_connect_keep,
                          _cpu_gen(drop_connect_keep, seed, offset),
                          shadow=shadow, ema=ema, ema_decay=ema_decay,
                          offset=offset, clip_coef=clip_coef, iters=iters)
        if zero_grad:
            grad.zero_()
    return master
