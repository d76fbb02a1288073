"""Device-resident evaluation.

The held-out set stays on the device as uint8 (a DeviceDataSet); one
evaluation is

  reset the accumulators and the cursor
  ceil(N_local / B) x { range_gather(cursor) -> model(x, train=False)
                        -> softmax_eval(..., cursor) }
  ONE read of the statistics

with no per-chunk host sync and no per-chunk host tensor.  The chunk body
has a fixed shape (the last chunk is padded with label -1 rows, which the
statistics kernel ignores) and all of its moving state lives in device
memory, so on a GPU in bf16 it is captured once into its own hipGraph and
replayed.  The graph reads the model's shadow weights in place: a weight
update between two evaluations needs no re-capture.

Model-agnostic (lenet and mlp: forward(x, train=False) -> [B, C] logits
with C = len(fc2_b) <= 16) and device-agnostic: on the CPU in fp32 the
same loop runs the reference ops (ops/cpu_ref.py) eagerly.
"""

from __future__ import annotations

import logging
import os
from typing import NamedTuple

import torch
import torch.distributed as dist

from ..ops import functional as Fx

log = logging.getLogger("dmnist.eval")


class EvalResult(NamedTuple):
    num_examples: int
    precision: float
    loss: float
    confusion: torch.Tensor  # int64 [C, C] on the host, rows = true class


class DeviceEvaluator:
    """Evaluates `model` on `dataset`, this rank's DeviceDataSet shard.

    With world > 1 every rank evaluates its own shard (build the data set
    with worker_id=rank, n_workers=world) and the statistics are summed
    with exactly one all_reduce per evaluation, outside any capture; every
    rank returns the full result.  All ranks must call run() together.
    """

    def __init__(self, model, dataset, batch_size: int, device, rank: int = 0,
                 world: int = 1):
        self.model = model
        self.ds = dataset
        self.B = int(batch_size)
        if self.B < 1:
            raise ValueError("eval batch size must be >= 1")
        self.device = torch.device(device)
        self.rank, self.world = rank, world
        if dataset.images.device != next(model.parameters()).device:
            raise ValueError(
                f"dataset lives on {dataset.images.device}, model on "
                f"{next(model.parameters()).device}")
        self.C = int(model.fc2_b.shape[0])  # both models end in fc2
        if not 1 <= self.C <= 16:
            raise ValueError(f"softmax_eval supports C <= 16, model has {self.C}")
        self.n_chunks = -(-dataset.num_examples // self.B)
        dev = dataset.images.device
        self.x = torch.zeros((self.B, 28, 28, 1), dtype=dataset.dtype,
                             device=dev)
        self.y = torch.full((self.B,), -1, dtype=torch.int64, device=dev)
        # one int32 block holds all running state, so a reset is one fill
        # and the read-back one copy: [cursor (int64) | loss_sum (fp32) |
        # counts (2 + C*C int32)]
        self._state = torch.zeros(3 + 2 + self.C * self.C, dtype=torch.int32,
                                  device=dev)
        self.cursor = self._state[0:2].view(torch.int64)
        self.loss_sum = self._state[2:3].view(torch.float32)
        self.counts = self._state[3:]
        self.graph = None
        if (dev.type == "cuda" and dataset.dtype == torch.bfloat16
                and self.n_chunks > 0
                and os.environ.get("DMNIST_EVAL_GRAPH", "1") != "0"):
            try:
                self.graph = self._capture()
            except Exception as e:  # noqa: BLE001 — eager on any failure
                log.warning("eval hipGraph capture unavailable (%s); "
                            "running eager", e)
                self.graph = None

    # -- one chunk ---------------------------------------------------------
    def _chunk(self):
        """gather at the cursor -> forward -> statistics (advances the
        cursor); device work only."""
        self.ds.range_into(self.x, self.y, start_dev=self.cursor)
        with torch.no_grad():
            logits = self.model(self.x, train=False)
        Fx.softmax_eval(logits, self.y, self.loss_sum, self.counts,
                        cursor_dev=self.cursor)

    def _capture(self):
        """Capture the chunk body (GraphedStep's hygiene: side-stream
        warm-up, collector off during capture, capture_end + stream restore
        on failure).  The warm-up runs touch only the chunk slots and the
        accumulators, which reset() clears."""
        import gc
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(2):
                self._chunk()
        cur.wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        # a dead Trainer <-> GraphedStep cycle freed by the collector in the
        # middle of a capture aborts the process (engine/graphstep.py)
        gc.collect()
        gc_was_enabled = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(graph):
                self._chunk()
        except Exception:
            try:
                graph.capture_end()
            except Exception:
                pass
            torch.cuda.set_stream(cur)
            raise
        finally:
            if gc_was_enabled:
                gc.enable()
        self.reset()
        torch.cuda.synchronize()
        return graph

    # -- public ------------------------------------------------------------
    def reset(self):
        self._state.zero_()

    def step_chunk(self):
        """Evaluate the next B examples (a chunk past the end is all
        padding and changes nothing)."""
        if self.graph is not None:
            self.graph.replay()
        else:
            self._chunk()

    def result(self) -> EvalResult:
        """Read the statistics: one D2H copy, one all_reduce at world > 1."""
        C = self.C
        if self.world > 1 and dist.is_initialized():
            # fp64 carries the int32 counts exactly, so loss and counts
            # travel in one collective
            red = torch.cat([self.loss_sum.double(), self.counts.double()])
            if red.is_cuda and dist.get_backend() != "nccl":
                red = red.cpu()
            dist.all_reduce(red, op=dist.ReduceOp.SUM)
            red = red.cpu()
            loss_sum = float(red[0])
            counts = red[1:].round().to(torch.int64)
        else:
            state = self._state.cpu()
            loss_sum = float(state[2:3].view(torch.float32))
            counts = state[3:].to(torch.int64)
        n, correct = int(counts[0]), int(counts[1])
        return EvalResult(n, correct / n if n else 0.0,
                          loss_sum / n if n else 0.0,
                          counts[2:].view(C, C).clone())

    def run(self) -> EvalResult:
        self.reset()
        for _ in range(self.n_chunks):
            self.step_chunk()
        return self.result()
