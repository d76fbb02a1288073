#!/usr/bin/env python3
"""Flagship benchmark: MNIST LeNet-5 CNN synchronous data-parallel SGD.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N>1
launched under `torch.distributed.run --nnodes=1 --nproc-per-node N`, one
rank per GPU over RCCL.  W untimed warmup steps, then EXACTLY K timed steps
bracketed by barrier + torch.cuda.synchronize on both sides; elapsed is the
MAX over ranks; rank 0 prints ONE JSON line.

A plain run does only what the headline figure needs: set up, warm up, time
the K steps, print the line.  `--full` adds the secondary measurements (the
separately sampled, per-step-synced p50/p95/p99 latency distribution).
`--dump-outputs DIR` writes what the last timed step returned (loss,
accuracy) and the parameters it left behind as DIR/<name>.npy.  Inputs and
initial weights are seeded, and with this option the last timed step starts
from the initial weights again, so the dump is one fwd+bwd+update of fixed
inputs: equal from run to run up to reduction-order rounding, and two builds
can be compared output for output.

Metric (BASELINE.json): images/sec whole node + p50 step time, MNIST CNN
sync-SGD, synthetic MNIST-shaped data, random-init weights, bf16 compute on
GPU.  Weak scaling: per-GPU batch fixed (default 1024 -> global 8192 at
N=8, the reference's CDF-config batch, cfg/time_cdf_cfgs/*:62).
"""

import argparse
import json
import os
import time

import numpy as np
import torch
import torch.distributed as dist


DUMP_BUDGET_BYTES = 64 * 1000 * 1000


def dump_outputs(out_dir, tensors):
    """Write each tensor as out_dir/<name>.npy (float32; float64 stays
    float64).  The whole dump stays under DUMP_BUDGET_BYTES: an array over
    its share is reduced to a fixed, seeded sample of its elements."""
    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_BUDGET_BYTES // max(1, len(tensors))
    for name, t in tensors.items():
        t = t.detach()
        t = t.to("cpu", torch.float64 if t.dtype == torch.float64
                 else torch.float32)
        a = np.ascontiguousarray(t.numpy())
        if a.nbytes > share:
            idx = np.random.default_rng(0).choice(
                a.size, size=share // a.itemsize, replace=False)
            a = a.reshape(-1)[np.sort(idx)]
        np.save(os.path.join(out_dir, f"{name}.npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None,
                    help="timed steps (default: 2000 GPU / 40 CPU so SMI "
                         "sampling sees a multi-second timed region)")
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--batch_size", type=int, default=1024,
                    help="per-GPU batch (weak scaling)")
    ap.add_argument("--model", default="lenet")
    ap.add_argument("--mode", default="full_sync",
                    choices=["full_sync", "k_of_n", "interval", "cdf"],
                    help="mapped onto the trainer's DP-mode flags (NOT "
                         "cosmetic: a cdf bench runs the cdf engine)")
    ap.add_argument("--replicas_to_aggregate", type=int, default=-1,
                    help="K for --mode k_of_n (-1 => world size)")
    ap.add_argument("--interval_ms", type=float, default=100.0,
                    help="aggregation period for --mode interval")
    ap.add_argument("--straggler", type=int, default=-1,
                    help="rank to slow down (straggler injection)")
    ap.add_argument("--straggler_ms", type=float, default=5.0,
                    help="per-step sleep on the injected rank")
    ap.add_argument("--straggler_timeout_ms", type=float, default=0.0,
                    help=">0: drop a rank's gradient past this deadline")
    ap.add_argument("--grad_dtype", default="fp32", choices=["fp32", "bf16"],
                    help="all-reduce wire dtype (fp32 master kept either way)")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements (per-step "
                         "synced p50/p95/p99 latency sampling); off by "
                         "default so a plain run times only the headline")
    ap.add_argument("--dump-outputs", dest="dump_outputs", default=None,
                    metavar="DIR",
                    help="write the last timed step's outputs (loss, "
                         "accuracy, updated parameters) as DIR/<name>.npy")
    args = ap.parse_args()
    on_gpu_probe = torch.cuda.is_available()
    if args.steps is None:
        # multi-second timed region by default so SMI utilization sampling
        # sees the run (round-1 BENCH carried gpu_busy=0.0 off one sample)
        args.steps = 5000 if on_gpu_probe else 40
    if args.warmup is None:
        args.warmup = 500 if on_gpu_probe else 10

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    on_gpu = torch.cuda.is_available()
    # modulo map so world_size > device_count still runs (e.g. exercising
    # the multi-rank path on a 1-GPU box); the driver's 8-GPU launch maps
    # 1:1.  DMNIST_BACKEND=gloo overrides RCCL for the same purpose.
    dev_idx = local_rank % max(1, torch.cuda.device_count()) if on_gpu else 0
    device = torch.device(f"cuda:{dev_idx}" if on_gpu else "cpu")
    if on_gpu:
        torch.cuda.set_device(device)
    if world > 1:
        backend = os.environ.get("DMNIST_BACKEND") or ("nccl" if on_gpu else "gloo")
        dist.init_process_group(backend, rank=rank, world_size=world)

    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser

    targv = [
        "--synthetic_data", "--model", args.model,
        "--batch_size", str(args.batch_size),
        "--train_dir", "/tmp/dmnist_bench",
        "--save_interval_secs", "100000",
        "--max_steps", str(args.steps + args.warmup + 60),
        "--grad_dtype", args.grad_dtype,
    ]
    # --mode maps onto the trainer's DP flags (reference mode semantics,
    # SURVEY.md section 2.2); the JSON "mode" field below is therefore the
    # mode that actually ran
    if args.mode == "cdf":
        targv += ["--worker_times_cdf_method"]
    elif args.mode == "interval":
        targv += ["--interval_method", "--interval_ms", str(args.interval_ms)]
    elif args.mode == "k_of_n":
        k = args.replicas_to_aggregate
        if k <= 0:
            k = max(1, int(os.environ.get("WORLD_SIZE", "1")) - 1)
        targv += ["--num_replicas_to_aggregate", str(k)]
    if args.straggler >= 0:
        targv += ["--inject_slow_rank", str(args.straggler),
                  "--inject_slow_ms", str(args.straggler_ms)]
    if args.straggler_timeout_ms > 0:
        targv += ["--straggler_timeout_ms", str(args.straggler_timeout_ms)]
    tflags = build_train_parser().parse_args(targv)
    trainer = Trainer(tflags, device=device, rank=rank, world=world,
                      local_rank=local_rank)
    trainer._num_examples = 60000
    ds = make_dataset(tflags, rank, world, trainer.device, trainer.compute_dtype)

    def one_step():
        x, y = ds.next_batch(args.batch_size)
        return trainer.graph_or_eager_step(x, y)

    # --dump-outputs: the kernels reduce with fp32 atomics, so each step
    # differs from run to run in the last bits, and hundreds of SGD steps on
    # random labels amplify that far beyond rounding.  To make the dump
    # comparable run to run (and build to build), the LAST timed step starts
    # from the seeded initial parameters again: its batch, step counter and
    # dropout stream are functions of the arguments alone, so what it
    # returns is one full fwd+bwd+update of fixed inputs.
    init_state = None
    if args.dump_outputs:
        init_state = (trainer.fp.flat_master.clone(),
                      None if trainer.flat_momentum is None
                      else trainer.flat_momentum.clone())
    dump_at = args.steps - 1 if init_state is not None else -1

    for _ in range(args.warmup):
        one_step()

    if world > 1:
        dist.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for i in range(args.steps):
        if i == dump_at:
            # the checkpoint-restore path: master, bf16 shadows, transposes
            trainer.fp.load_flat(init_state[0])
            if init_state[1] is not None:
                trainer.flat_momentum.copy_(init_state[1])
        last = one_step()
    if on_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0

    if args.dump_outputs and rank == 0 and last is not None:
        # snapshot now: loss/acc are static graph buffers and the parameters
        # keep training if --full samples more steps below
        _applied, loss_t, acc_t, _ct = last
        dump_outputs(args.dump_outputs, {
            "loss": loss_t, "accuracy": acc_t,
            "params": trainer.fp.flat_master})

    # per-step latency distribution, sampled SEPARATELY with a device sync
    # per step (graph replays enqueue asynchronously, so un-synced per-step
    # wall times are enqueue latencies, not step latencies); the headline
    # elapsed/steps above stays free of per-step sync overhead
    # (--full only: it is 30 more steps a plain run does not need)
    latency = {}
    if args.full:
        n_sample = min(args.steps, 30)
        step_t = np.zeros(n_sample)
        for i in range(n_sample):
            ts = time.perf_counter()
            one_step()
            if on_gpu:
                torch.cuda.synchronize()
            step_t[i] = time.perf_counter() - ts
        latency = {
            f"p{p}_ms_per_step": round(float(np.percentile(step_t, p)) * 1000, 4)
            for p in (50, 95, 99)}
    if trainer.mode == "interval":
        # drain outstanding interval aggregations so every rank leaves the
        # communicator with a matched collective count
        for grad, c in trainer.engine.finalize_interval():
            trainer._apply_update(grad, c)
    if world > 1:
        dist.barrier()
        t = torch.tensor([elapsed], dtype=torch.float64, device=device if on_gpu else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    n_gpus = world if world > 1 else args.gpus
    ms_per_step = elapsed / args.steps * 1000.0
    images_per_sec = args.batch_size * n_gpus * args.steps / elapsed
    dtype = "bf16" if trainer.compute_dtype == torch.bfloat16 else "fp32"
    if rank == 0:
        print(json.dumps({
            "metric": "images/sec (whole node), MNIST CNN sync-SGD",
            "value": round(images_per_sec, 1),
            "unit": "images/sec",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": dtype,
            "data": "synthetic",
            "config": {
                "model": args.model,
                "global_batch": args.batch_size * n_gpus,
                "seq_len": None,
                "parallelism": f"dp{n_gpus}",
                **latency,
                # the engine mode that actually ran (k_of_n degenerates to
                # full_sync at world=1 — reported honestly, never relabeled)
                "mode": trainer.mode,
                "mode_requested": args.mode,
                "grad_dtype": args.grad_dtype,
            },
        }), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
