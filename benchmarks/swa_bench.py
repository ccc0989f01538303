#!/usr/bin/env python
"""Sliding-window attention kernel benchmark at Mistral-7B head shapes
(H=32, Hkv=8, D=128, W=4096, 16-token KV pages).

Event-timed kernel calls, window against full context:

  decode   ops.attention_decode   B = 1, 8, 64   bf16 KV and fp8 KV
  prefill  ops.attention (dense)  B = 1          bf16

at context lengths 4k, 8k, 16k and 32k. Bytes per call are the bytes the
algorithm must read and write, computed from the shapes (K and V rows of
the keys a query may see, fp8 scales, q and out); TB/s is those bytes over
the measured time. Prefill also reports TFLOP/s over the visible
(query, key) pairs.

--baseline-so PATH loads a second build of the kernel library (for
instance the previous commit's) and times its full-context kernels in the
same process, alternating with this build's round by round, so the two
medians and their run-to-run spread come from the same minutes on the same
device.

Needs a GPU: there is no CPU fallback for a timing.
"""

import argparse
import importlib.machinery
import importlib.util
import json
import math
import statistics
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

H, HKV, D, WINDOW, PAGE = 32, 8, 128, 4096, 16
CONTEXTS = (4096, 8192, 16384, 32768)
DECODE_BATCHES = (1, 8, 64)


def load_ext(path):
    loader = importlib.machinery.ExtensionFileLoader("_hip_ops", path)
    spec = importlib.util.spec_from_loader("_hip_ops", loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


def decode_bytes(b, ctx, window, fp8):
    keys = min(ctx, window) if window else ctx
    item = 1 if fp8 else 2
    kv = 2 * b * keys * HKV * D * item
    scales = 2 * b * keys * HKV * 4 if fp8 else 0
    table = b * (keys // PAGE + 1) * 4
    qo = 2 * b * H * D * 2
    return kv + scales + table + qo


def visible_pairs(s, window):
    if not window or window >= s:
        return s * (s + 1) // 2
    return window * (window + 1) // 2 + (s - window) * window


def prefill_bytes(s):
    return (2 * H + 2 * HKV) * s * D * 2  # q + out, k + v


def prefill_flops(s, window):
    return 4 * visible_pairs(s, window) * H * D  # QK^T and PV


def time_rounds(variants, rounds, iters):
    """variants: {name: fn}. Alternates the variants round by round; each
    round times ``iters`` back-to-back calls between two device events.
    Returns {name: [ms per call, one entry per round]}."""
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


def summarise(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms),
            "max_ms": max(ms)}


def fmt(row):
    s = "{kernel:8s} {kv:5s} B={batch:<3d} ctx={ctx:<6d} {variant:14s} " \
        "{median_ms:9.4f} ms  [{min_ms:.4f} .. {max_ms:.4f}]  " \
        "{gbytes:8.3f} GB  {tbps:6.3f} TB/s".format(**row)
    if "tflops" in row:
        s += "  {:7.1f} TFLOP/s".format(row["tflops"])
    return s


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--baseline-so", default=None,
                    help="another build of _hip_ops.so to time alongside")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--contexts", type=int, nargs="*", default=CONTEXTS)
    ap.add_argument("--batches", type=int, nargs="*", default=DECODE_BATCHES)
    ap.add_argument("--out", default=None, help="also write the table here")
    args = ap.parse_args()

    if not torch.cuda.is_available():
        sys.exit("swa_bench: needs a GPU (no CPU fallback for timings)")
    import clearml_serving_amd.ops as ops

    if not ops.has_extension():
        sys.exit("swa_bench: HIP extension not built")
    base = load_ext(args.baseline_so) if args.baseline_so else None
    dev = "cuda:0"
    scale = 1.0 / math.sqrt(D)
    torch.manual_seed(0)
    rows, lines = [], []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    emit("# swa_bench: H={} Hkv={} D={} W={} page={}  device={}".format(
        H, HKV, D, WINDOW, PAGE, torch.cuda.get_device_name(0)))
    emit("# median of {} rounds x {} calls, [min .. max] over rounds; "
         "variants alternate round by round".format(args.rounds, args.iters))

    # ---------------- decode ---------------- #
    max_b, max_ctx = max(args.batches), max(args.contexts)
    pages = max_b * (max_ctx // PAGE)
    kf = torch.empty(pages, HKV, PAGE, D, device=dev,
                     dtype=torch.bfloat16).normal_()
    vf = torch.empty_like(kf).normal_()
    k8 = torch.randint(0, 120, kf.shape, device=dev, dtype=torch.uint8)
    v8 = torch.randint(0, 120, kf.shape, device=dev, dtype=torch.uint8)
    ks = torch.rand(pages, HKV, PAGE, device=dev) * 0.01 + 0.01
    vs = torch.rand(pages, HKV, PAGE, device=dev) * 0.01 + 0.01
    perm = torch.randperm(pages, device=dev).to(torch.int32)
    for fp8 in (False, True):
        kc, vc = (k8, v8) if fp8 else (kf, vf)
        sc = (ks, vs) if fp8 else (None, None)
        for b in args.batches:
            q = torch.randn(b, H, D, device=dev, dtype=torch.bfloat16)
            for ctx in args.contexts:
                nb = ctx // PAGE
                bt = perm[:b * nb].reshape(b, nb).contiguous()
                sl = torch.full((b,), ctx, dtype=torch.int32, device=dev)
                variants = {
                    "window": lambda: ops.attention_decode(
                        q, kc, vc, bt, sl, scale, sc[0], sc[1],
                        window=WINDOW),
                    "full": lambda: ops.attention_decode(
                        q, kc, vc, bt, sl, scale, sc[0], sc[1]),
                }
                if base is not None:
                    variants["full-baseline"] = lambda: base.attention_decode(
                        q, kc, vc, bt, sl, scale, sc[0], sc[1])
                iters = args.iters if b * ctx < 2 ** 20 else max(
                    args.iters // 4, 3)
                times = time_rounds(variants, args.rounds, iters)
                for name, ms in times.items():
                    nbytes = decode_bytes(
                        b, ctx, WINDOW if name == "window" else 0, fp8)
                    row = {"kernel": "decode", "kv": "fp8" if fp8 else "bf16",
                           "batch": b, "ctx": ctx, "variant": name,
                           "gbytes": nbytes / 1e9, **summarise(ms)}
                    row["tbps"] = nbytes / (row["median_ms"] * 1e-3) / 1e12
                    rows.append(row)
                    emit(fmt(row))
    del kf, vf, k8, v8, ks, vs

    # ---------------- prefill (dense, B=1) ---------------- #
    for ctx in args.contexts:
        qkv = torch.randn(1, ctx, H + 2 * HKV, D, device=dev,
                          dtype=torch.bfloat16)
        q, k, v = qkv.split([H, HKV, HKV], dim=2)
        variants = {
            "window": lambda: ops.attention(q, k, v, causal=True, scale=scale,
                                            layout="bshd", window=WINDOW),
            "full": lambda: ops.attention(q, k, v, causal=True, scale=scale,
                                          layout="bshd"),
        }
        if base is not None:
            variants["full-baseline"] = lambda: base.attention_prefill(
                q, k, v, True, scale, None, True)
        times = time_rounds(variants, args.rounds, max(args.iters // 4, 3))
        for name, ms in times.items():
            w = WINDOW if name == "window" else 0
            row = {"kernel": "prefill", "kv": "bf16", "batch": 1, "ctx": ctx,
                   "variant": name, "gbytes": prefill_bytes(ctx) / 1e9,
                   **summarise(ms)}
            row["tbps"] = prefill_bytes(ctx) / (row["median_ms"] * 1e-3) / 1e12
            row["tflops"] = prefill_flops(ctx, w) / (
                row["median_ms"] * 1e-3) / 1e12
            rows.append(row)
            emit(fmt(row))

    # ---------------- window-off vs baseline ---------------- #
    if base is not None:
        emit("# full context, this build vs baseline build "
             "(ratio of medians; spread = (max - min) / median per variant)")
        by = {(r["kernel"], r["kv"], r["batch"], r["ctx"], r["variant"]): r
              for r in rows}
        for r in rows:
            if r["variant"] != "full":
                continue
            key = (r["kernel"], r["kv"], r["batch"], r["ctx"])
            o = by[key + ("full-baseline",)]
            emit("{:8s} {:5s} B={:<3d} ctx={:<6d} this/baseline {:6.3f}  "
                 "spread this {:5.1%}  baseline {:5.1%}".format(
                     *key, r["median_ms"] / o["median_ms"],
                     (r["max_ms"] - r["min_ms"]) / r["median_ms"],
                     (o["max_ms"] - o["min_ms"]) / o["median_ms"]))

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"bench": "swa", "rows": rows}))


if __name__ == "__main__":
    main()
