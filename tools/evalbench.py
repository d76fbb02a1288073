#!/usr/bin/env python3
"""Evaluation-throughput benchmark (bench.py measures training only).
Generates a 10000-image idx-gz test set from a seed and times one full
evaluation of one fixed LeNet three ways:

  a  do_eval      engine/evaluate.py::do_eval at its default chunk: fp32
                  host tensors, pageable H2D + cast, training softmax,
                  two host syncs per chunk (the polling evaluator's path)
  b  eager        DeviceEvaluator with DMNIST_EVAL_GRAPH=0
  c  graph        DeviceEvaluator, chunk body replayed from its hipGraph

Every variant is warmed up, then timed over `--evals` whole evaluations
between two device events with one synchronise at the end (each evaluation
ends in its own statistics read-back; that is part of its cost).  The
variants alternate inside each of `--repeats` rounds so drift hits all of
them alike; the spread over the rounds is reported next to every ratio.
Prints one JSON line.  Needs a GPU: there is no fallback.
"""

import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = {"a": "do_eval_host_fed", "b": "device_eval_eager",
            "c": "device_eval_graph"}


def timed(fn, reps):
    """Seconds for `reps` calls, by device events around the whole window
    (host-bound stretches leave the device idle inside it: that is the
    cost)."""
    import torch
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1000.0


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n_test", type=int, default=10000)
    ap.add_argument("--eval_batch_size", type=int, default=1000)
    ap.add_argument("--evals", type=int, default=200,
                    help="whole evaluations per timed window (about 1 ms "
                         "each: 200 make a window of a fifth of a second)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=66478)
    ap.add_argument("--out", default="", help="also write the JSON here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("evalbench: no GPU visible; this tool measures the device "
                 "evaluation path and has no CPU fallback")
    from distributedmnist_amd.data import load_device_mnist, load_mnist
    from distributedmnist_amd.data.mnist_data import write_random_idx
    from distributedmnist_amd.engine.device_eval import DeviceEvaluator
    from distributedmnist_amd.engine.evaluate import do_eval
    from distributedmnist_amd.models import build_model
    from distributedmnist_amd.parallel import FlatParams

    device, dtype = torch.device("cuda:0"), torch.bfloat16
    model = build_model("lenet", seed=args.seed,
                        compute_dtype=dtype).to(device)
    FlatParams(model, device=device, compute_dtype=dtype)
    with tempfile.TemporaryDirectory(prefix="evalbench_") as tmp:
        write_random_idx(tmp, 64, args.n_test, seed=args.seed)
        host = load_mnist(tmp, shard=False).validation
        resident = load_device_mnist(tmp, shard=False, device=device,
                                     dtype=dtype, split="test")
    # what evaluate() hands do_eval for every checkpoint
    images = torch.as_tensor(host.images)
    labels = torch.as_tensor(host.labels)

    os.environ["DMNIST_EVAL_GRAPH"] = "0"
    ev_eager = DeviceEvaluator(model, resident, args.eval_batch_size, device)
    os.environ["DMNIST_EVAL_GRAPH"] = "1"
    ev_graph = DeviceEvaluator(model, resident, args.eval_batch_size, device)
    if ev_eager.graph is not None or ev_graph.graph is None:
        sys.exit("evalbench: the eager/graph evaluators did not come up as "
                 "asked; refusing to time the wrong path")
    fns = {"a": lambda: do_eval(model, images, labels, device, dtype),
           "b": ev_eager.run, "c": ev_graph.run}
    outs = {}
    for k, fn in fns.items():
        for _ in range(args.warmup):
            outs[k] = fn()
    torch.cuda.synchronize()
    ips = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, fn in fns.items():  # alternate the variants inside each round
            ips[k].append(round(
                args.n_test * args.evals / timed(fn, args.evals), 1))
    result = {"metric": "images_per_sec", "model": "lenet",
              "device": torch.cuda.get_device_name(0),
              "n_test": args.n_test,
              "eval_batch_size": args.eval_batch_size,
              "do_eval_chunk": 10000, "evals_per_window": args.evals,
              "warmup": args.warmup, "repeats": args.repeats,
              "variants": VARIANTS,
              "precision": {"a": outs["a"][0], "b": outs["b"].precision,
                            "c": outs["c"].precision},
              "loss": {"a": outs["a"][1], "b": outs["b"].loss,
                       "c": outs["c"].loss}}
    for k, v in ips.items():
        result[k] = dict(spread(v), runs=v)
    for num, den in (("c", "a"), ("b", "a"), ("c", "b")):
        result[f"{num}/{den}"] = spread(
            [round(x / y, 4) for x, y in zip(ips[num], ips[den])])
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
