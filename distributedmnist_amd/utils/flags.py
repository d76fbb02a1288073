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


def build_train_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="MI355X-native distributed MNIST training")
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
    p.add_argument("--grad_dtype", default="fp32", choices=["fp32", "bf16"],
                   help="all-reduce wire dtype: bf16 halves the xGMI payload "
                        "(6.65->3.33 MB); the fp32 master update is unchanged")
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
