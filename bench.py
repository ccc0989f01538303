#!/usr/bin/env python3
"""Flagship serving benchmark (driver contract).

Measures the BASELINE.json headline metric: requests/sec (+ p50 latency) for
ResNet-50 and BERT-base endpoints with dynamic auto-batching, bf16, synthetic
data, random-init weights, on N GPUs of one node.

One rank per GPU (torch.distributed over RCCL); each rank runs an independent
serving replica (data-parallel serving = the reference's N-workers topology,
entrypoint.sh:56-72) -- weak scaling. Each *step* pushes a fixed burst of
requests through the full serving path (ModelRequestProcessor dispatch ->
dynamic batcher -> hipGraph replay on the GPU) and awaits all responses.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints one JSON result
line. ``--dump-outputs DIR`` also writes the responses of the last timed
step as ``DIR/<endpoint>.npy`` (float32, request order; inputs are seeded, so
two builds can be compared output for output). A plain run warms up only the
batch buckets its steps can form (step_buckets()); ``--full`` warms every
serving-default bucket and adds the per-endpoint batcher telemetry on stderr.
"""

import argparse
import asyncio
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

REQ_PER_STEP = int(os.environ.get("CMLS_BENCH_REQ", 512))
# per rank per step: REQ/2 ResNet-50 + REQ/2 BERT-base requests


DUMP_MAX_BYTES = 64 << 20  # cap on everything --dump-outputs writes


_T_START = time.perf_counter()


def log(msg):
    if int(os.environ.get("RANK", 0)) == 0:
        print("[bench +{:.1f}s] {}".format(time.perf_counter() - _T_START,
                                           msg), file=sys.stderr, flush=True)


def dump_outputs(out_dir, collected):
    """Write the last timed step's responses, one float32 array per endpoint
    (row i = response to that endpoint's i-th request of the step). Arrays
    that would push the total past DUMP_MAX_BYTES are cut to a fixed, seeded
    sample of rows (sorted, so row order stays request order)."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    budget = DUMP_MAX_BYTES // max(len(collected), 1)
    for name, rows in sorted(collected.items()):
        arr = np.stack([np.asarray(rows[i], dtype=np.float32)
                        for i in sorted(rows)])
        if arr.nbytes > budget:
            keep = max(budget // max(arr[0].nbytes, 1), 1)
            idx = np.sort(np.random.default_rng(1234).choice(
                arr.shape[0], size=min(keep, arr.shape[0]), replace=False))
            arr = arr[idx]
        np.save(os.path.join(out_dir, name + ".npy"), arr)
        log("dumped {}.npy {}".format(name, arr.shape))


MAX_BATCH = 64


def step_buckets():
    """Batch buckets one step can form from its REQ_PER_STEP/2 requests per
    endpoint: full MAX_BATCH batches plus the bucket that holds the
    remainder. A plain run warms up (MIOpen find + hipGraph capture) only
    these; --full keeps every serving-default bucket."""
    from clearml_serving_amd.serving.batcher import DEFAULT_BUCKETS

    n = REQ_PER_STEP // 2
    buckets = {MAX_BATCH} if n >= MAX_BATCH else set()
    if n % MAX_BATCH:
        buckets.add(next(b for b in sorted(DEFAULT_BUCKETS) + [MAX_BATCH]
                         if b >= n % MAX_BATCH))
    return sorted(buckets) or [MAX_BATCH]


def build_processor(device_idx, tmpdir, use_graphs=True, buckets=None):
    from clearml_serving_amd.schemas import ModelEndpoint
    from clearml_serving_amd.serving.processor import ModelRequestProcessor
    from clearml_serving_amd.store import ServingStore

    store = ServingStore(os.path.join(tmpdir, "store"))
    processor = ModelRequestProcessor(store=store, name="bench",
                                      force_create=True)
    processor._metric_log_freq = 0.0  # stats sampling off in the bench

    cards = {
        "resnet50_bench": {"arch": "resnet50", "num_classes": 1000,
                           "dtype": "bfloat16"},
        "bert_bench": {"arch": "bert-base", "num_labels": 2,
                       "dtype": "bfloat16"},
    }
    specs = {
        "resnet50_bench": dict(input_size=[3, 224, 224], input_type="float32"),
        "bert_bench": dict(input_size=[[128], [128]],
                           input_type=["int64", "int32"],
                           input_name=["input_ids", "attention_mask"]),
    }
    for name, card in cards.items():
        p = os.path.join(tmpdir, name + ".json")
        with open(p, "wt") as f:
            json.dump(card, f)
        rec = store.register_model(name=name, project="bench", path=p)
        processor.add_endpoint(ModelEndpoint(
            engine_type="hip", serving_url=name, model_id=rec.model_id,
            auxiliary_cfg={
                "max_batch_size": MAX_BATCH,
                "max_queue_delay_us": 4000,
                "dtype": "bfloat16" if torch.cuda.is_available() else "float32",
                "use_graphs": use_graphs,
                "gpu": device_idx,
                # None: the serving default (every bucket warmed up)
                "preferred_batch_size": buckets,
            },
            **specs[name],
        ))
    return processor


async def run_step(processor, resnet_inputs, bert_inputs, latencies=None,
                   checksum=None, offset=0, collect=None):
    """One bench step: REQ_PER_STEP requests through the serving path.

    ``offset`` rotates through the input pools so consecutive steps see
    different request tensors (no caching artifacts); ``checksum``
    accumulates a scalar over every response (outputs are consumed, and the
    total is printed with the result for cross-run comparison); ``collect``
    (dict) keeps every response as collect[endpoint][i] for --dump-outputs."""

    async def one(endpoint, body, i):
        t0 = time.perf_counter()
        out = await processor.process_request(endpoint, "", body)
        if latencies is not None:
            latencies.append(time.perf_counter() - t0)
        if checksum is not None:
            import numpy as np

            arr = np.asarray(out, dtype=np.float64)
            checksum[0] += float(arr.sum())
            checksum[1] += arr.size
        if collect is not None:
            collect.setdefault(endpoint, {})[i] = out

    tasks = []
    n = REQ_PER_STEP // 2
    for i in range(n):
        j = (offset + i) % len(resnet_inputs)
        tasks.append(one("resnet50_bench", resnet_inputs[j], i))
        tasks.append(one("bert_bench", bert_inputs[j], i))
    await asyncio.gather(*tasks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults sized for a >=60 s steady-state timed region on one MI355X
    # (~40 ms/step measured); still finishes within minutes
    ap.add_argument("--steps", type=int, default=1600)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--no-graphs", action="store_true")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's responses as "
                         "DIR/<endpoint>.npy (float32, rank 0 only)")
    ap.add_argument("--full", action="store_true",
                    help="warm up every serving-default batch bucket and "
                         "report per-endpoint batcher telemetry")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    has_gpu = torch.cuda.is_available()

    dist = None
    if world > 1:
        import torch.distributed as dist_mod

        dist = dist_mod
        backend = "nccl" if has_gpu else "gloo"
        dist.init_process_group(backend=backend)
        if has_gpu:
            torch.cuda.set_device(local_rank)

    device_idx = local_rank if has_gpu else 0

    # synthetic requests of the headline shapes (BASELINE.json configs 2+3):
    # ResNet-50: [3, 224, 224] bf16; BERT-base: seq_len 128 token ids
    torch.manual_seed(1234 + rank)
    # per-request unique tensors: the pool is larger than any batch window,
    # and run_step rotates its offset so steps never repeat a request lineup
    n_distinct = int(os.environ.get("CMLS_BENCH_DISTINCT", 256))
    dtype = torch.bfloat16 if has_gpu else torch.float32
    resnet_inputs = [torch.randn(3, 224, 224, dtype=dtype)
                     for _ in range(n_distinct)]
    bert_inputs = [
        {"input_ids": torch.randint(0, 30000, (128,), dtype=torch.int64),
         "attention_mask": torch.ones(128, dtype=torch.int32)}
        for _ in range(n_distinct)
    ]

    with tempfile.TemporaryDirectory() as tmpdir:
        processor = build_processor(
            device_idx, tmpdir, use_graphs=not args.no_graphs and has_gpu,
            buckets=None if args.full else step_buckets())

        loop = asyncio.new_event_loop()
        asyncio.set_event_loop(loop)

        log("warmup: {} steps (includes hipGraph capture per bucket)".format(
            args.warmup))
        for w in range(max(args.warmup, 1)):
            loop.run_until_complete(
                run_step(processor, resnet_inputs, bert_inputs,
                         offset=w * 13))

        log("timed: {} steps".format(args.steps))
        # ---- timed region: barrier + sync on both sides ---- #
        if dist:
            dist.barrier()
        if has_gpu:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        latencies = []
        checksum = [0.0, 0]
        collected = {} if (args.dump_outputs and rank == 0) else None
        for k in range(args.steps):
            loop.run_until_complete(
                run_step(processor, resnet_inputs, bert_inputs, latencies,
                         checksum=checksum, offset=k * 13,
                         collect=(collected if k == args.steps - 1
                                  else None)))
        if has_gpu:
            torch.cuda.synchronize()
        if dist:
            dist.barrier()
        elapsed = time.perf_counter() - t0

        # slowest rank defines job time
        if dist:
            t = torch.tensor([elapsed], dtype=torch.float64,
                             device="cuda" if has_gpu else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())

        total_requests = world * args.steps * REQ_PER_STEP
        rps = total_requests / elapsed
        p50 = statistics.median(latencies) * 1000 if latencies else None
        p99 = (sorted(latencies)[int(len(latencies) * 0.99)] * 1000
               if latencies else None)

        if collected:
            dump_outputs(args.dump_outputs, collected)

        if rank == 0:
            result = {
                "metric": "requests/sec + p50 latency, ResNet-50 & BERT-base "
                          "dyn-batch, 1/2/4/8 MI355X",
                "value": round(rps, 2),
                "unit": "requests/s",
                "n_gpus": world,
                "steps": args.steps,
                "warmup": args.warmup,
                "ms_per_step": round(elapsed / args.steps * 1000, 3),
                "higher_is_better": True,
                "scaling": "weak",
                "vs_baseline": None,
                "dtype": "bf16" if has_gpu else "fp32",
                "data": "synthetic",
                "config": {
                    "model": "resnet50+bert-base",
                    "global_batch": REQ_PER_STEP * world,
                    "seq_len": 128,
                    "image": "3x224x224",
                    "parallelism": "dp{}".format(world),
                    "max_batch_size": MAX_BATCH,
                    "p50_latency_ms": round(p50, 2) if p50 else None,
                    "p99_latency_ms": round(p99, 2) if p99 else None,
                    "requests_per_step": REQ_PER_STEP,
                    "timed_region_s": round(elapsed, 2),
                    "output_checksum": round(checksum[0], 3),
                    "outputs_consumed": checksum[1],
                },
            }
            print(json.dumps(result), flush=True)

        # per-endpoint batcher telemetry to stderr (optimization guidance)
        telemetry = (processor._engine_processor_lookup.items()
                     if args.full else ())
        for url, eng in telemetry:
            b = getattr(eng, "_batcher", None)
            if b is not None and b.stats["batches"]:
                s = b.stats
                log("{}: batches={} occupancy={:.2f} stage_ms/b={:.2f} "
                    "gpu_wait_ms/b={:.2f}".format(
                        url, s["batches"],
                        s["occupancy_sum"] / s["batches"],
                        s["stage_ms_sum"] / s["batches"],
                        s["gpu_wait_ms_sum"] / s["batches"]))
        processor.stop()
        if dist:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
