#!/usr/bin/env python3
"""Real-data input-pipeline benchmark (bench.py measures --synthetic_data
only).  Generates MNIST-sized idx-gz files from a seed, then times one
LeNet training step fed five ways, per batch size:

  a  host    DataSet.next_batch -> Trainer.to_device -> graph_or_eager_step
  b  eager   --device_data --hip_graph off  (resident_step, eager gather)
  c  graph   --device_data                  (gather captured in the hipGraph)
  d  synth   --synthetic_data               (graph; device slices + 2 copies)
  e  augment --device_data --augment_shift 2 --augment_rotate 10
             --augment_scale 0.1            (graph; warped gather captured)

Every variant is warmed up at its shape, then timed over `--steps` steps
between two device events with ONE synchronise at the end and no per-step
host read-back.  The variants alternate inside each of `--repeats` rounds so
drift hits all of them alike; the spread over the rounds is reported next
to every ratio.  Prints one JSON line.  Needs a GPU: there is no fallback.
"""

import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = {
    "a": ("host_fed_graph", []),
    "b": ("device_data_eager", ["--device_data", "--hip_graph", "off"]),
    "c": ("device_data_graph", ["--device_data"]),
    "d": ("synthetic_graph", ["--synthetic_data"]),
    "e": ("device_data_augment_graph",
          ["--device_data", "--augment_shift", "2", "--augment_rotate", "10",
           "--augment_scale", "0.1"]),
}


def build_variant(key, data_dir, train_dir, batch_size, seed):
    """-> (trainer, zero-arg step function)."""
    import torch
    from distributedmnist_amd.data import DeviceDataSet
    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    flags = build_train_parser().parse_args(
        ["--model", "lenet", "--batch_size", str(batch_size),
         "--data_dir", data_dir, "--train_dir", train_dir,
         "--seed", str(seed), "--save_interval_secs", "100000",
         *VARIANTS[key][1]])
    t = Trainer(flags, device=torch.device("cuda:0"))
    ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
    t._num_examples = ds.num_examples
    if isinstance(ds, DeviceDataSet):
        t.attach_dataset(ds)
        return t, t.resident_step
    if key == "a":
        def step():
            x, y = ds.next_batch(batch_size)
            return t.graph_or_eager_step(*t.to_device(x, y))
    else:
        def step():
            return t.graph_or_eager_step(*ds.next_batch(batch_size))
    return t, step


def timed(step, steps):
    """Seconds for `steps` steps, by device events around the whole window
    (for a host-bound feed the device idles inside it: that is the cost)."""
    import torch
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1000.0


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch_sizes", default="64,1024")
    ap.add_argument("--variants", default="a,b,c,d,e")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n_train", type=int, default=60000)
    ap.add_argument("--seed", type=int, default=66478)
    ap.add_argument("--out", default="", help="also write the JSON here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("databench: no GPU visible; this tool measures the device "
                 "input path and has no CPU fallback")
    from distributedmnist_amd.data.mnist_data import write_random_idx

    keys = [k for k in args.variants.split(",") if k]
    batch_sizes = [int(b) for b in args.batch_sizes.split(",")]
    result = {"metric": "images_per_sec", "model": "lenet",
              "device": torch.cuda.get_device_name(0),
              "n_train": args.n_train, "steps": args.steps,
              "warmup": args.warmup, "repeats": args.repeats,
              "variants": {k: VARIANTS[k][0] for k in keys}, "batch": {}}
    with tempfile.TemporaryDirectory(prefix="databench_") as tmp:
        data_dir = os.path.join(tmp, "data")
        write_random_idx(data_dir, args.n_train, 1000, seed=args.seed)
        for bs in batch_sizes:
            steps_fn = {}
            for k in keys:
                t, fn = build_variant(k, data_dir, os.path.join(tmp, "td"),
                                      bs, args.seed)
                for _ in range(args.warmup):
                    fn()
                torch.cuda.synchronize()
                graphed = t._graph is not None
                if graphed != (k != "b"):
                    sys.exit(f"databench: variant {k} at B={bs} "
                             f"{'did' if graphed else 'did not'} capture a "
                             "hipGraph; refusing to time the wrong path")
                steps_fn[k] = fn
            ips = {k: [] for k in keys}
            for _ in range(args.repeats):
                for k in keys:  # alternate the variants inside each round
                    ips[k].append(round(
                        bs * args.steps / timed(steps_fn[k], args.steps), 1))
            entry = {k: dict(spread(v), runs=v) for k, v in ips.items()}
            for num, den in (("c", "a"), ("c", "d"), ("e", "c")):
                if num in ips and den in ips:
                    entry[f"{num}/{den}"] = spread(
                        [round(x / y, 4) for x, y in zip(ips[num], ips[den])])
            result["batch"][str(bs)] = entry
            del steps_fn
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
