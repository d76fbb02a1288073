"""Hand-scheduled LeNet training step (GPU bf16 path).

Replaces autograd's serial backward with an explicit schedule; used inside
the hipGraph capture (graphstep.py).

Backward dataflow (both pool backwards fused into their consumers: neither
pre-pool gradient, dact1 or dact2, is ever written to memory):

  a1 --> fc2 head: logits, softmax(+db2), dW2, dx2+mask+db1 = dyeff1
           (one kernel; logits and dlogits stay in LDS)
              dyeff1 --> dW1
              dyeff1 --> dX+poolmask = gp2 [B,7,7,64] (+db_conv2)
                (gp2, am2) --> conv2 dW   (dact2 rebuilt in the LDS slab)
                (gp2, am2) --> conv2 dX = dxc --> conv1 dW+db (pooled)
All dW/db land directly in the flat fp32 all-reduce bucket (zeroed by the
SGD tail of the previous step).

DMNIST_POOL2_FUSED=0 selects the earlier three calls, which materialise the
dense dact2 [B,14,14,64] (dX+unpool -> conv_dw_into / conv_dx), for A/B.

Round-1 ran the dW chain on a SIDE stream overlapping the dX chain;
round-2 same-box A/B showed the single-stream schedule is ~7% faster
end-to-end at B<=2048 (cross-stream graph-edge semaphores + CU contention
on the dX chain outweigh the overlap there) while the overlap still wins at
B>=4096 — the schedule is batch-tiered (FusedLeNetStep.__init__).
"""

from __future__ import annotations

import torch
import torch.distributed as dist

from .. import _C


class FusedLeNetStep:
    def __init__(self, trainer):
        t = trainer
        m = t.model
        from ..models import LeNet5
        assert isinstance(m, LeNet5), "fused step is LeNet-specific"
        assert t.compute_dtype == torch.bfloat16 and t.device.type == "cuda"
        assert m.shadows and m.shadows_T, "fused step needs bf16 shadows"
        self.t = t
        self.ext = _C.ext()
        # Stream schedule is BATCH-TIERED (same-box A/B, after the
        # per-call side-stream fix): at B=1024 the cross-stream fork/join
        # edges of the replayed graph plus the dW kernels' CU contention on
        # the dX chain cost more than the overlap buys (0.429 two-stream vs
        # 0.400 ms single; 0.384 after the conv1-dW G retune); at B=8192
        # the hidden dW work dominates the edge cost (1.698 vs 1.733) —
        # single-stream below 4096, overlapped above.  DMNIST_TWO_STREAM /
        # DMNIST_SINGLE_STREAM force either for A/B.
        # overlap level: 0 = single stream, 1 = fc dW only on the side
        # stream (cheap contention, conv2 dW serial), 2 = every dW on the
        # side stream (round-1 schedule).  DMNIST_OVERLAP=0/1/2 forces;
        # legacy DMNIST_TWO_STREAM=1 -> 2, DMNIST_SINGLE_STREAM=1 -> 0.
        import os as _os
        if _os.environ.get("DMNIST_OVERLAP"):
            self.overlap_level = int(_os.environ["DMNIST_OVERLAP"])
        elif _os.environ.get("DMNIST_TWO_STREAM"):
            self.overlap_level = 2
        elif _os.environ.get("DMNIST_SINGLE_STREAM"):
            self.overlap_level = 0
        else:
            self.overlap_level = 0 if t.flags.batch_size < 4096 else 2
        self.single_stream = self.overlap_level == 0
        # pool2 backward inside the conv2 dX / dW staging (gp2 + am2, no
        # dense dact2); DMNIST_POOL2_FUSED=0 keeps the dX+unpool route
        self.pool2_fused = _os.environ.get("DMNIST_POOL2_FUSED", "1") != "0"
        # side stream resolved PER CALL: in single-stream mode it must be
        # whatever stream the body is running on RIGHT NOW (warmup and
        # graph capture run on their own streams — freezing the init-time
        # stream here sent the dW ops to a foreign stream with no
        # dependency edges: silent gradient races)
        self.side = None if self.single_stream else torch.cuda.Stream()
        self.p_keep = 0.5
        self.seed = t.flags.seed
        # bucketed all-reduce: the fc gradients (96.5% of the payload,
        # SURVEY.md §2.4) are complete long before the conv backward — their
        # collective overlaps it on the side stream.  The flat bucket layout
        # (conv*, then fc*) makes the split two contiguous slices.
        fp = t.fp
        fc0 = fp.offsets[fp.names.index("fc1_w")]
        self.fc_offset = fc0
        self.conv_slice = fp.flat_grad[:fc0]
        self.fc_slice = fp.flat_grad[fc0:]
        self.overlap_allreduce = t.world > 1 and dist.is_initialized()

    def _fork(self, a, b):
        """a.wait_stream(b), elided in single-stream mode (each edge is a
        semaphore pair in the captured graph)."""
        if not self.single_stream:
            a.wait_stream(b)

    def __call__(self, x, labels, step_dev):
        """One fwd+bwd; gradients land in the flat bucket.
        Returns (loss, mean_accuracy) device scalars."""
        reduce_grads = self.overlap_allreduce
        loss, acc, conv_in, self._keep = self._fc_part(x, labels, step_dev,
                                                       reduce_grads)
        self._conv_part(*conv_in)
        if reduce_grads:
            self.t.engine.wire_allreduce(self.conv_slice, start=0)
        return loss, acc

    # ------------------------------------------------------------------
    # Two-stage form of the SAME schedule, for the two-graph split capture
    # (graphstep.py): stage_fc ends with every fc gradient final (so the
    # eager fc-slice all-reduce can launch between the graphs and overlap
    # stage_conv's replay); stage_conv finishes the conv backward.  Both
    # forms run _fc_part then _conv_part; here the collectives live OUTSIDE
    # and the fc stage joins its side stream at the end so graph A's
    # boundary is well-defined.
    def stage_fc(self, x, labels, step_dev):
        loss, acc, self._stash, self._keep = self._fc_part(
            x, labels, step_dev, False)
        s0, s1 = self._streams()
        s0.wait_stream(s1)  # graph A boundary: fc grads complete
        return loss, acc

    def stage_conv(self):
        self._conv_part(*self._stash)
        self._keep2 = self._stash

    def _gv(self, name):
        return getattr(self.t.model, name).grad

    def _streams(self):
        """(s0, s1): the stream the body runs on RIGHT NOW and the dW side
        stream (s0 itself in single-stream mode)."""
        s0 = torch.cuda.current_stream()
        return s0, (s0 if self.single_stream else self.side)

    def _fc_part(self, x, labels, step_dev, reduce_fc):
        """Forward, the fc2 head, fc1 dW, fc1 dX+poolmask.
        reduce_fc issues the fc-slice all-reduce on s1 right after fc1 dW.
        Returns (loss, acc, _conv_part's arguments, keep): keep holds every
        tensor a side-stream op of either part reads, and the caller stores
        it until the join (capture-safe)."""
        ext, gv = self.ext, self._gv
        m = self.t.model
        sh, shT = m.shadows, m.shadows_T
        B = x.shape[0]
        s0, s1 = self._streams()

        # ---- forward (s0) ----
        y1, am1 = ext.conv_pool_fwd(x, sh["conv1_w"], m.conv1_b, None)
        y2, am2 = ext.conv_pool_fwd(y1, sh["conv2_w"], m.conv2_b,
                                    shT["conv2_w"])
        h2 = y2.view(B, 7 * 7 * 64)
        a1 = ext.linear_act_fwd_dev(h2, sh["fc1_w"], m.fc1_b, True,
                                    self.p_keep, self.seed, step_dev,
                                    shT["fc1_w"])
        # the whole fc2 layer in one op (s0): forward, softmax (+ fc2 bias
        # grad, loss, MEAN accuracy via inv_n), fc2 dW, and fc2 dX with the
        # fc1 relu+dropout mask (+ fc1 bias grad).  One kernel by default;
        # the op itself falls back to the four separate launches
        # (DMNIST_FC2_FUSED=0, deterministic mode, uncovered shapes)
        loss, acc, dyeff1 = ext.fc2_head(a1, sh["fc2_w"], shT["fc2_w"],
                                         m.fc2_b, labels, gv("fc2_w"),
                                         gv("fc2_b"), gv("fc1_b"),
                                         self.p_keep, 1.0 / B)

        # ---- backward: dX chain on s0, dW GEMMs on s1 ----
        self._fork(s1, s0)
        with torch.cuda.stream(s1):
            ext.linear_dw_into(h2, dyeff1, gv("fc1_w"))
            if reduce_fc:
                # every fc gradient (fc2's and the db's from the head on s0,
                # ordered by wait_stream) is final here
                self.t.engine.wire_allreduce(self.fc_slice,
                                             start=self.fc_offset)
        # fc1 dX with the pool2 mask + conv2 db in the GEMM epilogue
        # (liveness rides in the amax byte, no y2 re-read); pool2 backward
        # itself happens in the conv2 dW / dX slab staging.  conv2_b is in
        # the conv slice, reduced after the conv part in either form.
        g2 = self._fc1_dx(dyeff1, am2)
        keep = (a1, h2, dyeff1, y1, g2, am2)
        return loss, acc, (x, y1, am1, g2, am2), keep

    def _conv_part(self, x, y1, am1, g2, am2):
        """conv2 dW (placed by overlap level), conv2 dX, conv1 dW+db, and
        the s0 <- s1 join."""
        s0, s1 = self._streams()
        sW = s1 if self.overlap_level >= 2 else s0  # conv2 dW placement
        if sW is not s0:
            self._fork(sW, s0)
        with torch.cuda.stream(sW):
            self._conv2_dw(y1, g2, am2)
        dxc = self._conv2_dx(g2, am2)
        # conv1 dW+db consume the POOLED gradient (pool1 backward fused in
        # the consumer; the 4x-size dact1 is never materialized)
        self.ext.conv1_dw_pooled(x, dxc, am1, self._gv("conv1_w"),
                                 self._gv("conv1_b"))
        self._fork(s0, s1)

    # pool2 backward: g2 is the pooled gradient gp2 [B,7,7,64] (default) or,
    # with DMNIST_POOL2_FUSED=0, the dense dact2 [B,14,14,64]
    def _fc1_dx(self, dyeff1, am2):
        m = self.t.model
        f = (self.ext.linear_dx_pooled if self.pool2_fused
             else self.ext.linear_dx_unpool)
        return f(dyeff1, m.shadows["fc1_w"], am2, m.conv2_b.grad, 7, 7, 64)

    def _conv2_dw(self, y1, g2, am2):
        dw = self.t.model.conv2_w.grad
        if self.pool2_fused:
            self.ext.conv_dw_pooled_into(y1, g2, am2, dw)
        else:
            self.ext.conv_dw_into(y1, g2, dw)

    def _conv2_dx(self, g2, am2):
        w = self.t.model.shadows["conv2_w"]
        if self.pool2_fused:
            return self.ext.conv_dx_pooled(g2, am2, w, 32)
        return self.ext.conv_dx(g2, w, 32)
