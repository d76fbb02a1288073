"""Flag registry — argparse mirror of the reference's tf.app.flags surface
(/root/reference/src/distributed_train.py:36-99).

Reference flags are kept name-for-name so existing launch tooling maps over.
`ps_hosts` is accepted and ignored (there is no parameter server on an
8xMI355X node); `worker_hosts`/`task_id` are superseded by torchrun's
RANK/WORLD_SIZE env when present.  New MI355X-specific flags are grouped at
the bottom.
"""

from __future__ import annotations

import argparse
import os


def _decay(text: str) -> float:
    """--moving_average_decay: a float in [0, 1)."""
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {text!r}")
    if not 0.0 <= v < 1.0:  # also refuses nan
        raise argparse.ArgumentTypeError(
            f"must lie in [0, 1), got {text}")
    return v


def _clip(text: str) -> float:
    """--clip_grad_norm: 0 (off) or a threshold > 0, inf included."""
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {text!r}")
    if not v >= 0.0:  # also refuses nan
        raise argparse.ArgumentTypeError(
            f"must be 0 (off) or > 0 (inf = never clip), got {text}")
    return v


def _lars_eta(text: str) -> float:
    """--lars_eta: 0 (off) or a finite trust coefficient > 0."""
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {text!r}")
    if not 0.0 <= v < float("inf"):  # also refuses nan
        raise argparse.ArgumentTypeError(
            f"must be 0 (off) or finite and > 0, got {text}")
    return v


def _grad_topk(text: str) -> float:
    """--grad_topk: 0 (off) or a ratio in (0, 1]."""
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {text!r}")
    if not 0.0 <= v <= 1.0:  # also refuses nan
        raise argparse.ArgumentTypeError(
            f"must be 0 (off) or lie in (0, 1], got {text}")
    return v


def _grad_lowrank(text: str) -> int:
    """--grad_lowrank: 0 (off) or a rank in 1..16."""
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not an integer: {text!r}")
    if not 0 <= v <= 16:
        raise argparse.ArgumentTypeError(
            f"must be 0 (off) or lie in 1..16, got {text}")
    return v


def _adam_eps(text: str) -> float:
    """--adam_eps: finite and > 0."""
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {text!r}")
    if not 0.0 < v < float("inf"):  # also refuses nan
        raise argparse.ArgumentTypeError(
            f"must be finite and > 0, got {text}")
    return v


class _TrainParser(argparse.ArgumentParser):
    """Checks that span two flags, reported as argument errors."""

    def parse_known_args(self, args=None, namespace=None):
        ns, rest = super().parse_known_args(args, namespace)
        if ns.optimizer == "sgd":
            if ns.weight_decay > 0 and not ns.lars_eta > 0:
                self.error("argument --weight_decay: needs --lars_eta > 0 "
                           "(the decay is applied by the LARS update only) "
                           "or --optimizer adam|lamb")
            for name in ("adam_beta1", "adam_beta2", "adam_eps"):
                if getattr(ns, name) is not None:
                    self.error(f"argument --{name}: needs --optimizer "
                               "adam|lamb")
        elif ns.optimizer == "muon":
            # --momentum (its mu) and --weight_decay (decoupled) are legal
            if not 0.0 <= ns.momentum < 1.0:
                self.error("argument --momentum: must lie in [0, 1) with "
                           "--optimizer muon")
            if ns.lars_eta > 0:
                self.error("argument --lars_eta: not with --optimizer muon "
                           "(its update has a fixed norm per tensor)")
            for name in ("adam_beta1", "adam_beta2", "adam_eps"):
                if getattr(ns, name) is not None:
                    self.error(f"argument --{name}: needs --optimizer "
                               "adam|lamb")
        else:
            if ns.momentum > 0:
                self.error("argument --momentum: not with --optimizer "
                           f"{ns.optimizer} (beta1 is its momentum)")
            if ns.lars_eta > 0:
                self.error("argument --lars_eta: not with --optimizer "
                           f"{ns.optimizer} (lamb is the Adam-based LARS)")
        if ns.grad_topk > 0:
            # the sparse exchange replaces the dense synchronous all-reduce
            # only (the checks that need the world size: Trainer)
            for bad, what in (
                    (ns.interval_method, "--interval_method (the interval "
                     "accumulator is dense)"),
                    ((ns.straggler_timeout_ms or 0) > 0,
                     "--straggler_timeout_ms > 0 (a dropped payload would "
                     "lose its residual)"),
                    (ns.grad_dtype != "fp32", f"--grad_dtype {ns.grad_dtype} "
                     "(the payload is index + fp32 value pairs)")):
                if bad:
                    self.error(f"argument --grad_topk: not with {what}")
        if ns.grad_lowrank > 0:
            # as above: two small all-reduces replace the dense one
            for bad, what in (
                    (ns.grad_topk > 0, "--grad_topk (one compressor at a "
                     "time)"),
                    (ns.interval_method, "--interval_method (the interval "
                     "accumulator is dense)"),
                    ((ns.straggler_timeout_ms or 0) > 0,
                     "--straggler_timeout_ms > 0 (a dropped factor would "
                     "lose its residual)"),
                    (ns.grad_dtype != "fp32", f"--grad_dtype {ns.grad_dtype} "
                     "(the factors stay fp32)")):
                if bad:
                    self.error(f"argument --grad_lowrank: not with {what}")
        if ns.grad_dtype == "mxfp8":
            # the quantised reduce-scatter / all-gather replaces the dense
            # synchronous all-reduce only (the checks that need the world
            # size: Trainer)
            for bad, what in (
                    (ns.interval_method, "--interval_method (the interval "
                     "accumulator is dense)"),
                    ((ns.straggler_timeout_ms or 0) > 0,
                     "--straggler_timeout_ms > 0 (the contributor flag "
                     "cannot ride in a quantised buffer)")):
                if bad:
                    self.error(f"argument --grad_dtype mxfp8: not with {what}")
        # the defaults, once the "was it given" check is done
        for name, default in (("adam_beta1", 0.9), ("adam_beta2", 0.999),
                              ("adam_eps", 1e-8)):
            if getattr(ns, name) is None:
                setattr(ns, name, default)
        return ns, rest


def _in_range(lo: float, hi: float):
    """argparse type: a float in [lo, hi]."""
    def parse(text: str) -> float:
        try:
            v = float(text)
        except ValueError:
            raise argparse.ArgumentTypeError(f"not a number: {text!r}")
        if not lo <= v <= hi:  # also refuses nan
            raise argparse.ArgumentTypeError(
                f"must lie in [{lo:g}, {hi:g}], got {text}")
        return v
    return parse


def build_train_parser() -> argparse.ArgumentParser:
    p = _TrainParser(description="MI355X-native distributed MNIST training")
    # --- reference-compatible flags (distributed_train.py:36-99) ---
    p.add_argument("--worker_times_cdf_method", action="store_true",
                   help="collect per-worker compute-time CDFs (DP-2 mode)")
    p.add_argument("--interval_method", action="store_true",
                   help="wall-clock interval aggregation (DP-3 mode)")
    p.add_argument("--should_summarize", action="store_true",
                   help="write TensorBoard summaries on the chief")
    p.add_argument("--timeline_logging", action="store_true",
                   help="write per-step chrome traces (torch.profiler)")
    p.add_argument("--job_name", default="worker", choices=["ps", "worker"],
                   help="kept for CLI parity; 'ps' exits immediately (no PS on MI355X)")
    p.add_argument("--ps_hosts", default="", help="ignored (no parameter server)")
    p.add_argument("--worker_hosts", default="", help="comma-separated; superseded by torchrun env")
    p.add_argument("--train_dir", default="/tmp/mnist_train",
                   help="checkpoints + event logs directory")
    p.add_argument("--rpc_port", type=int, default=1235, help="vestigial (reference RPC mesh port)")
    p.add_argument("--save_results_period", type=int, default=20,
                   help="steps between worker time/accuracy npy dumps")
    p.add_argument("--max_steps", type=int, default=1000)
    p.add_argument("--drop_connect", action="store_true")
    p.add_argument("--batch_size", type=int, default=64, help="per-worker batch size")
    p.add_argument("--subset", type=int, default=0, help="train on a subset of N examples (0=all)")
    p.add_argument("--log_device_placement", action="store_true", help="vestigial")
    p.add_argument("--task_id", type=int, default=None,
                   help="worker rank; defaults to env RANK")
    p.add_argument("--num_replicas_to_aggregate", type=int, default=-1,
                   help="K of K-of-N aggregation; -1 => K = world size")
    p.add_argument("--save_interval_secs", type=int, default=20)
    p.add_argument("--save_summaries_secs", type=int, default=300)
    p.add_argument("--initial_learning_rate", type=float, default=0.01)
    p.add_argument("--momentum", type=float, default=0.0,
                   help="SGD momentum mu (0 = reference GradientDescent parity)")
    p.add_argument("--num_epochs_per_decay", type=float, default=1.0)
    p.add_argument("--learning_rate_decay_factor", type=float, default=0.95)
    p.add_argument("--drop_connect_probability", type=float, default=0.9,
                   help="keep probability of the per-element gradient mask")
    p.add_argument("--interval_ms", type=float, default=1000.0,
                   help="interval-method aggregation period")
    # --- MI355X-native additions ---
    p.add_argument("--model", default="lenet", choices=["lenet", "mlp"])
    p.add_argument("--synthetic_data", action="store_true",
                   help="device-resident synthetic MNIST-shaped data")
    p.add_argument("--fake_data", action="store_true", help="reference fake-data mode")
    p.add_argument("--data_dir", default="data", help="MNIST idx-gz directory")
    p.add_argument("--no_shard", action="store_true",
                   help="reference parity: every worker sees the full set")
    p.add_argument("--compute_dtype", default="auto", choices=["auto", "fp32", "bf16"],
                   help="auto => bf16 on GPU, fp32 on CPU")
    p.add_argument("--straggler_timeout_ms", type=float, default=0.0,
                   help=">0: drop own gradient when compute exceeds this (DP-4)")
    p.add_argument("--inject_slow_rank", type=int, default=-1,
                   help="rank to slow down for straggler testing")
    p.add_argument("--inject_slow_ms", type=float, default=0.0,
                   help="sleep this long per step on the injected rank")
    p.add_argument("--seed", type=int, default=66478)
    p.add_argument("--device", default="auto", help="auto|cpu|cuda")
    p.add_argument("--hip_graph", default="auto",
                   choices=["auto", "off", "full"],
                   help="capture the training step in a hipGraph (GPU full-sync)")
    p.add_argument("--fused_step", default="auto", choices=["auto", "off"],
                   help="hand-scheduled two-stream LeNet step inside the graph")
    p.add_argument("--backend", default="auto", help="auto|nccl|gloo")
    p.add_argument("--grad_dtype", default="fp32",
                   choices=["fp32", "bf16", "mxfp8"],
                   help="all-reduce wire dtype: bf16 halves the xGMI payload "
                        "(6.65->3.33 MB); the fp32 master update is "
                        "unchanged. mxfp8: OCP MXFP8 (e4m3 codes, one E8M0 "
                        "scale per 32 elements) with unbiased stochastic "
                        "rounding; a quantised reduce-scatter (all-to-all, "
                        "sum in fp32, requantise) and all-gather replace the "
                        "all-reduce and every rank decodes the same bytes. "
                        "With one rank the bucket is encoded and decoded in "
                        "place. Not with --grad_topk, --grad_lowrank, "
                        "--interval_method, --num_replicas_to_aggregate "
                        "below the world size, --straggler_timeout_ms or "
                        "--hip_graph full at world > 1")
    p.add_argument("--grad_topk", type=_grad_topk, default=0.0,
                   metavar="RATIO",
                   help="RATIO in (0, 1]: top-k gradient sparsification with "
                        "error feedback (Aji & Heafield 2017, Stich et al. "
                        "2018). Every rank adds its gradient to a local "
                        "residual, sends the ceil(RATIO * n) largest "
                        "magnitudes of every tensor as (index, value) pairs "
                        "(one all-gather) and keeps the rest in the "
                        "residual; the pairs are summed in rank order, so "
                        "all ranks hold the same bits. Selected on the "
                        "device by a radix select in a fixed order. Not "
                        "with --interval_method, --num_replicas_to_aggregate "
                        "below the world size, --straggler_timeout_ms, "
                        "--grad_dtype bf16 or --hip_graph full at world > 1. "
                        "0 = off")
    p.add_argument("--grad_lowrank", type=_grad_lowrank, default=0,
                   metavar="R",
                   help="R in 1..16: PowerSGD rank-R gradient compression "
                        "with error feedback (Vogels, Karimireddy, Jaggi "
                        "2019). Every weight matrix the kernels can tile "
                        "(rows and cols multiples of 16, 64..4096 x 64..512) "
                        "is sent as two thin fp32 factors in two small "
                        "all-reduces, whatever the world size; what the "
                        "factors miss stays in a local residual. All other "
                        "tensors are sent exactly. fp32 MFMA kernels with "
                        "fixed summation orders. Not with --grad_topk, "
                        "--interval_method, --num_replicas_to_aggregate below "
                        "the world size, --straggler_timeout_ms, --grad_dtype "
                        "bf16 or --hip_graph full at world > 1. 0 = off")
    p.add_argument("--drop_connect_post", action="store_true",
                   help="legacy round-1 form: one shared mask on the "
                        "AGGREGATED gradient (default is the reference's "
                        "per-worker pre-aggregation masks, "
                        "distributed_train.py:194-203)")
    p.add_argument("--device_data", action="store_true",
                   help="keep the idx-gz training set on the device as uint8 "
                        "and gather each batch there (inside the hipGraph "
                        "when the step is captured); the batch order is a "
                        "pure function of (seed, rank, step). No effect "
                        "with --synthetic_data / --fake_data")
    p.add_argument("--augment_shift", type=float, default=0.0, metavar="PX",
                   help=">0 (with --device_data): random translation of "
                        "every training image by up to PX pixels per axis, "
                        "inside the resident gather; the transform is a pure "
                        "function of (seed, rank, step, batch position)")
    p.add_argument("--augment_rotate", type=float, default=0.0, metavar="DEG",
                   help=">0 (with --device_data): random rotation by up to "
                        "DEG degrees about the image centre")
    p.add_argument("--augment_scale", type=float, default=0.0, metavar="FRAC",
                   help=">0 (with --device_data): random log-uniform scaling "
                        "in [1/(1+FRAC), 1+FRAC]")
    p.add_argument("--augment_table", type=int, default=4096, metavar="T",
                   help="number of distinct random transforms the augmented "
                        "gather draws from (built once per rank)")
    p.add_argument("--augment_elastic", type=_in_range(0.0, 64.0),
                   default=0.0, metavar="ALPHA",
                   help=">0 (with --device_data): elastic distortion (Simard "
                        "et al. 2003) of every training image inside the "
                        "resident gather: a random displacement field of up "
                        "to ALPHA pixels (<= 64), smoothed by a Gaussian; a "
                        "pure function of (seed, rank, step, batch position). "
                        "Combines with the affine flags; 0 = off")
    p.add_argument("--augment_elastic_sigma", type=_in_range(1.0, 16.0),
                   default=4.0, metavar="S",
                   help="standard deviation in pixels, in [1, 16], of the "
                        "Gaussian that smooths the elastic field")
    p.add_argument("--eval_every_steps", type=int, default=0,
                   help=">0: keep the test set on the device and evaluate it "
                        "every N steps (and after the last step); the step "
                        "line's test_acc and column 2 of the time/accuracy "
                        "npy carry the most recent precision. Not with "
                        "--interval_method")
    p.add_argument("--eval_batch_size", type=int, default=1000,
                   help="chunk size of the in-training evaluation")
    p.add_argument("--moving_average_decay", type=_decay, default=0.0,
                   metavar="D",
                   help="D in (0, 1): keep an exponential moving average of "
                        "the weights (update k uses min(D, (1+k)/(10+k)), "
                        "TensorFlow's ExponentialMovingAverage with "
                        "num_updates), updated inside the SGD kernel, saved "
                        "in the checkpoint as flat_ema and used by "
                        "--eval_every_steps; 0 = off")
    p.add_argument("--clip_grad_norm", type=_clip, default=0.0, metavar="C",
                   help="C > 0: scale the aggregated (averaged) gradient by "
                        "min(1, C / (global L2 norm + 1e-6)) before the "
                        "update, torch.nn.utils.clip_grad_norm_ semantics; "
                        "the norms are reduced on the device in a fixed "
                        "order (no host round trip, same bits on every "
                        "rank). inf never clips and only reports the norms; "
                        "0 = off")
    p.add_argument("--lars_eta", type=_lars_eta, default=0.0, metavar="ETA",
                   help="ETA > 0: layer-wise adaptive rate scaling (LARS, You "
                        "et al. 2017). Every weight tensor's step is scaled "
                        "by ETA * |w| / (|g| + WD * |w|), the norms reduced "
                        "on the device in one launch in a fixed order (no "
                        "host round trip, same bits on every rank); biases "
                        "are left alone. With --clip_grad_norm the same "
                        "launch also clips. 0 = off")
    p.add_argument("--weight_decay", type=_in_range(0.0, float("inf")),
                   default=0.0, metavar="WD",
                   help="L2 weight decay of the LARS update (weight tensors "
                        "only): g += WD * w inside the trust ratio and the "
                        "step. Needs --lars_eta. With --optimizer adam: "
                        "decoupled AdamW decay, w -= lr * WD * w (the same "
                        "with --optimizer muon); with "
                        "--optimizer lamb: u += WD * w before the trust ratio")
    p.add_argument("--optimizer", choices=("sgd", "adam", "lamb", "muon"),
                   default="sgd",
                   help="sgd: the fused SGD pass (--momentum, --lars_eta). "
                        "adam: fused Adam / AdamW. lamb: LAMB (You et al. "
                        "2019), Adam's update scaled per weight tensor by "
                        "|w| / |update|, the norms reduced on the device in a "
                        "fixed order; biases get plain Adam. Both keep two "
                        "fp32 moment buffers (checkpointed as flat_adam_m / "
                        "flat_adam_v); not with --momentum or --lars_eta. "
                        "muon: Nesterov momentum (--momentum) whose update of "
                        "every weight tensor is orthogonalised by five "
                        "Newton-Schulz iterations on the matrix cores, "
                        "decoupled --weight_decay; biases get plain momentum; "
                        "not with --lars_eta or --adam_*")
    p.add_argument("--adam_beta1", type=_decay, default=None, metavar="B1",
                   help="first-moment decay in [0, 1) (default 0.9)")
    p.add_argument("--adam_beta2", type=_decay, default=None, metavar="B2",
                   help="second-moment decay in [0, 1) (default 0.999)")
    p.add_argument("--adam_eps", type=_adam_eps, default=None, metavar="EPS",
                   help="added to sqrt(v) (default 1e-8); finite and > 0")
    p.add_argument("--deterministic", action="store_true",
                   help="bitwise-reproducible gradients on the GPU: the fused "
                        "LeNet step reduces every weight and bias gradient "
                        "in a fixed order (per-block planes + an ordered "
                        "reduction) instead of fp32 atomics; routes that are "
                        "not covered raise. Not with --interval_method, "
                        "--num_replicas_to_aggregate below the world size or "
                        "--straggler_timeout_ms; accepted and a no-op on CPU")
    return p


def build_eval_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="MI355X-native MNIST evaluator")
    # reference flags (nn_eval.py:36-44, mnist_eval.py)
    p.add_argument("--eval_dir", default="/tmp/mnist_eval")
    p.add_argument("--checkpoint_dir", default="/tmp/mnist_train")
    p.add_argument("--eval_interval_secs", type=int, default=30)
    p.add_argument("--run_once", action="store_true")
    p.add_argument("--fake_data", action="store_true")
    p.add_argument("--synthetic_data", action="store_true")
    p.add_argument("--data_dir", default="data")
    p.add_argument("--model", default="lenet", choices=["lenet", "mlp"])
    p.add_argument("--device", default="auto")
    p.add_argument("--max_evals", type=int, default=0, help="0 = run forever")
    p.add_argument("--device_data", action="store_true",
                   help="keep the test set on the device as uint8 and "
                        "evaluate every checkpoint there (model and buffers "
                        "built once, checkpoints loaded in place)")
    p.add_argument("--eval_batch_size", type=int, default=1000,
                   help="chunk size of the --device_data evaluation")
    p.add_argument("--use_moving_average", action="store_true",
                   help="evaluate the checkpoint's weight moving average "
                        "(flat_ema, written by training runs with "
                        "--moving_average_decay) instead of the raw weights; "
                        "an error on checkpoints without one")
    p.add_argument("--confusion", action="store_true",
                   help="with --device_data: also save "
                        "eval_dir/confusion-<step>.npy and log per-class "
                        "recall")
    return p


def resolve_rank_world(flags) -> tuple[int, int]:
    """torchrun env wins; else task_id/worker_hosts; else single process."""
    if "RANK" in os.environ and "WORLD_SIZE" in os.environ:
        return int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    world = len(flags.worker_hosts.split(",")) if flags.worker_hosts else 1
    rank = flags.task_id if flags.task_id is not None else 0
    return rank, world
