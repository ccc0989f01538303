#!/usr/bin/env python
"""Speculative-verification attention benchmark at Llama-3-8B head shapes
(H=32, Hkv=8, D=128, 16-token KV pages).

For every (KV dtype, B, context, Sq) point, three ways to attend Sq
in-flight query tokens per sequence to a paged context, event-timed in the
same run and alternating round by round:

  multi    ops.attention_decode_multi   the split-KV multi-query kernel
  paged    ops.attention_prefill_paged  the chunked-prefill kernel, which
                                        verification used before
  decode   Sq calls of ops.attention_decode, one per query token

`context` is the number of keys the LAST query token sees. Bytes per call
are what the algorithm must move (the K and V rows and fp8 scales of the
context once per kv head, block table, q and out); TB/s is those bytes over
the measured median. The closing table lists multi/paged per point: the
engine routes verification to the new kernel only where that ratio is below
one (LlmEngine._verify_attn_route).

Needs a GPU: there is no CPU fallback for a timing.
"""

import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

H, HKV, D, PAGE = 32, 8, 128, 16
BATCHES = (1, 4, 8)
CONTEXTS = (32, 128, 1024, 4096, 16384)  # 32, 128: short end of the routing
QUERIES = (2, 5, 8)


def moved_bytes(b, ctx, sq, fp8):
    kv = 2 * b * ctx * HKV * D * (1 if fp8 else 2)
    scales = 2 * b * ctx * HKV * 4 if fp8 else 0
    table = b * (ctx // PAGE) * 4
    qo = 2 * b * sq * H * D * 2
    return kv + scales + table + qo


def time_rounds(variants, rounds, iters):
    """Alternates the variants round by round; a round times ``iters``
    back-to-back calls between two device events. {name: [ms per call]}."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            start = torch.cuda.Event(enable_timing=True)
            stop = torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(iters):
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) / iters)
    return times


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batches", type=int, nargs="*", default=BATCHES)
    ap.add_argument("--contexts", type=int, nargs="*", default=CONTEXTS)
    ap.add_argument("--queries", type=int, nargs="*", default=QUERIES)
    ap.add_argument("--out", default=None, help="also write the table here")
    args = ap.parse_args()

    if not torch.cuda.is_available():
        sys.exit("verify_attn_bench: needs a GPU (no CPU fallback for "
                 "timings)")
    import clearml_serving_amd.ops as ops

    if not ops.has_extension():
        sys.exit("verify_attn_bench: HIP extension not built")
    dev = "cuda:0"
    scale = 1.0 / math.sqrt(D)
    torch.manual_seed(0)
    rows, lines = [], []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    emit("# verify_attn_bench: H={} Hkv={} D={} page={}  device={}".format(
        H, HKV, D, PAGE, torch.cuda.get_device_name(0)))
    emit("# median of {} rounds x {} calls, [min .. max] over rounds; the "
         "three variants alternate round by round".format(
             args.rounds, args.iters))

    max_b, max_ctx = max(args.batches), max(args.contexts)
    pages = max_b * (max_ctx // PAGE)
    kf = torch.empty(pages, HKV, PAGE, D, device=dev,
                     dtype=torch.bfloat16).normal_()
    vf = torch.empty_like(kf).normal_()
    k8 = torch.randint(0, 120, kf.shape, device=dev, dtype=torch.uint8)
    v8 = torch.randint(0, 120, kf.shape, device=dev, dtype=torch.uint8)
    ks = torch.full((pages, HKV, PAGE), 2.0 ** -6, device=dev)
    vs = ks.clone()
    perm = torch.randperm(pages, device=dev).to(torch.int32)
    for fp8 in (False, True):
        kc, vc = (k8, v8) if fp8 else (kf, vf)
        sc = (ks, vs) if fp8 else (None, None)
        for b in args.batches:
            for ctx in args.contexts:
                nb = ctx // PAGE
                bt = perm[:b * nb].reshape(b, nb).contiguous()
                kl = torch.full((b,), ctx, dtype=torch.int32, device=dev)
                for sq in args.queries:
                    q = torch.randn(b, sq, H, D, device=dev,
                                    dtype=torch.bfloat16)
                    ql = torch.full((b,), sq, dtype=torch.int32, device=dev)
                    step_lens = [kl - (sq - 1 - j) for j in range(sq)]

                    def decode_calls():
                        for j in range(sq):
                            ops.attention_decode(q[:, j], kc, vc, bt,
                                                 step_lens[j], scale,
                                                 sc[0], sc[1])

                    variants = {
                        "multi": lambda: ops.attention_decode_multi(
                            q, kc, vc, bt, kl, ql, scale, sc[0], sc[1]),
                        "paged": lambda: ops.attention_prefill_paged(
                            q, kc, vc, bt, kl, ql, scale, sc[0], sc[1]),
                        "decode": decode_calls,
                    }
                    times = time_rounds(variants, args.rounds, args.iters)
                    nbytes = moved_bytes(b, ctx, sq, fp8)
                    for name, ms in times.items():
                        row = {"kv": "fp8" if fp8 else "bf16", "batch": b,
                               "ctx": ctx, "sq": sq, "variant": name,
                               "median_ms": statistics.median(ms),
                               "min_ms": min(ms), "max_ms": max(ms),
                               "gbytes": nbytes / 1e9}
                        row["tbps"] = nbytes / (row["median_ms"] * 1e-3) / 1e12
                        rows.append(row)
                        emit("{kv:5s} B={batch:<2d} ctx={ctx:<6d} Sq={sq:<2d}"
                             " {variant:7s} {median_ms:9.4f} ms  "
                             "[{min_ms:.4f} .. {max_ms:.4f}]  "
                             "{gbytes:7.4f} GB  {tbps:6.3f} TB/s".format(
                                 **row))

    emit("# ratio of medians per point (below 1: the multi-query kernel "
         "is faster)")
    by = {(r["kv"], r["batch"], r["ctx"], r["sq"], r["variant"]): r
          for r in rows}
    for r in rows:
        if r["variant"] != "multi":
            continue
        key = (r["kv"], r["batch"], r["ctx"], r["sq"])
        emit("{:5s} B={:<2d} ctx={:<6d} Sq={:<2d} multi/paged {:6.3f}  "
             "multi/decode {:6.3f}".format(
                 *key, r["median_ms"] / by[key + ("paged",)]["median_ms"],
                 r["median_ms"] / by[key + ("decode",)]["median_ms"]))

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"bench": "verify_attn", "rows": rows}))


if __name__ == "__main__":
    main()
