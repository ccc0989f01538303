#!/usr/bin/env python3
"""Per-kernel microbenchmarks on MI355X (run under gpurun).

Reports achieved TFLOP/s (attention) and GB/s (memory-bound ops) so kernel
iterations can be compared run to run. Usage:
    python benchmarks/kernel_bench.py [--csv out.csv]
"""

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import clearml_serving_amd.ops as ops  # noqa: E402


def timeit(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_attention(results):
    for (b, h, s, d) in [(16, 12, 128, 64), (8, 12, 384, 64),
                         (16, 32, 1024, 128), (8, 32, 2048, 128)]:
        q = torch.randn(b, h, s, d, device="cuda", dtype=torch.bfloat16)
        k = torch.randn_like(q)
        v = torch.randn_like(q)
        dt = timeit(lambda: ops.attention(q, k, v))
        flops = 4.0 * b * h * s * s * d  # QK^T + PV
        results.append(dict(op="attention_prefill",
                            shape="b{}h{}s{}d{}".format(b, h, s, d),
                            us=dt * 1e6, tflops=flops / dt / 1e12))
        dtc = timeit(lambda: ops.attention(q, k, v, causal=True))
        results.append(dict(op="attention_prefill_causal",
                            shape="b{}h{}s{}d{}".format(b, h, s, d),
                            us=dtc * 1e6, tflops=0.5 * flops / dtc / 1e12))


def bench_decode(results):
    bs = 16
    for (b, h, hkv, d, seq) in [(32, 32, 8, 128, 1024), (64, 32, 8, 128, 2048),
                                (128, 32, 8, 128, 4096)]:
        nb = b * ((seq + bs - 1) // bs)
        k_cache = torch.randn(nb, hkv, bs, d, device="cuda",
                              dtype=torch.bfloat16)
        v_cache = torch.randn_like(k_cache)
        bt = torch.arange(nb, dtype=torch.int32, device="cuda").reshape(b, -1)
        sl = torch.full((b,), seq, dtype=torch.int32, device="cuda")
        q = torch.randn(b, h, d, device="cuda", dtype=torch.bfloat16)
        dt = timeit(lambda: ops.attention_decode(q, k_cache, v_cache, bt, sl))
        bytes_moved = 2.0 * b * hkv * seq * d * 2  # K+V read, bf16
        results.append(dict(op="attention_decode",
                            shape="b{}h{}hkv{}d{}s{}".format(b, h, hkv, d, seq),
                            us=dt * 1e6, gbps=bytes_moved / dt / 1e9))


def bench_memops(results):
    for (rows, h) in [(8192, 768), (16384, 4096), (4096, 8192)]:
        x = torch.randn(rows, h, device="cuda", dtype=torch.bfloat16)
        w = torch.randn(h, device="cuda", dtype=torch.bfloat16)
        b = torch.randn(h, device="cuda", dtype=torch.bfloat16)
        r = torch.randn_like(x)
        dt = timeit(lambda: ops.layernorm(x, w, b, residual=r))
        bytes_moved = x.numel() * 2 * 3  # read x + r, write out
        results.append(dict(op="layernorm_residual",
                            shape="{}x{}".format(rows, h),
                            us=dt * 1e6, gbps=bytes_moved / dt / 1e9))
        dt = timeit(lambda: ops.rmsnorm(x, w))
        results.append(dict(op="rmsnorm", shape="{}x{}".format(rows, h),
                            us=dt * 1e6,
                            gbps=x.numel() * 2 * 2 / dt / 1e9))

    x = torch.randn(16384, 3072, device="cuda", dtype=torch.bfloat16)
    bb = torch.randn(3072, device="cuda", dtype=torch.bfloat16)
    dt = timeit(lambda: ops.bias_gelu(x, bb))
    results.append(dict(op="bias_gelu", shape="16384x3072", us=dt * 1e6,
                        gbps=x.numel() * 2 * 2 / dt / 1e9))

    g = torch.randn(8192, 14336, device="cuda", dtype=torch.bfloat16)
    u = torch.randn_like(g)
    dt = timeit(lambda: ops.silu_mul(g, u))
    results.append(dict(op="silu_mul", shape="8192x14336", us=dt * 1e6,
                        gbps=g.numel() * 2 * 3 / dt / 1e9))

    x = torch.randn(4, 64, 56, 56 * 64, device="cuda", dtype=torch.bfloat16)
    r = torch.randn_like(x)
    dt = timeit(lambda: ops.bias_relu_add(x, residual=r))
    results.append(dict(op="relu_add", shape="4x64x56x3584", us=dt * 1e6,
                        gbps=x.numel() * 2 * 3 / dt / 1e9))


def bench_gemm(results):
    for (m, n, k) in [(4096, 4096, 4096), (8192, 8192, 8192),
                      (8192, 3072, 768)]:
        a = torch.randn(m, k, device="cuda", dtype=torch.bfloat16)
        b = torch.randn(n, k, device="cuda", dtype=torch.bfloat16)
        dt = timeit(lambda: ops.gemm_bf16(a, b), iters=20)
        results.append(dict(op="gemm_bf16(ours)",
                            shape="{}x{}x{}".format(m, n, k),
                            us=dt * 1e6, tflops=2.0 * m * n * k / dt / 1e12))
        dtl = timeit(lambda: a @ b.T, iters=20)
        results.append(dict(op="gemm_hipblaslt",
                            shape="{}x{}x{}".format(m, n, k),
                            us=dtl * 1e6, tflops=2.0 * m * n * k / dtl / 1e12))


def bench_sampling(results):
    logits = torch.randn(64, 128256, device="cuda", dtype=torch.bfloat16)
    dt = timeit(lambda: ops.sample_top_k_top_p(logits, temperature=0.8))
    results.append(dict(op="sample_gumbel", shape="64x128256", us=dt * 1e6,
                        gbps=logits.numel() * 2 / dt / 1e9))


def bench_lora(results):
    """Multi-LoRA decode step: shrink + expand (csrc/lora.hip) at T=64 rows
    over L=4 adapters of rank 16, for the four merged llama-3-8b
    projections, next to the eager torch composition of the same math
    (index_select + bmm + add)."""
    t, nl, r = 64, 4, 16
    h, q_out, kv_out, inter = 4096, 4096, 1024, 14336
    idx = (torch.arange(t, device="cuda") % nl).to(torch.int32)
    sel = idx.long()
    for name, k, n, parts in [("qkv", h, q_out + 2 * kv_out, 3),
                              ("o_proj", q_out, h, 1),
                              ("gate_up", h, 2 * inter, 2),
                              ("down", inter, h, 1)]:
        rr = parts * r  # A matrices of a merged projection stack along rank
        x = torch.randn(t, k, device="cuda", dtype=torch.bfloat16)
        a = torch.randn(nl, rr, k, device="cuda", dtype=torch.bfloat16) \
            * k ** -0.5
        b = torch.randn(nl, n, rr, device="cuda", dtype=torch.bfloat16)
        out = torch.zeros(t, n, device="cuda", dtype=torch.bfloat16)

        def ours():
            ops.lora_expand_add(ops.lora_shrink(x, a, idx), b, idx, out)

        def eager():
            y = torch.bmm(a.index_select(0, sel), x.unsqueeze(-1))
            out.add_(torch.bmm(b.index_select(0, sel), y).squeeze(-1))

        # per-token A and B rows + x read + out read/write
        bytes_moved = 2.0 * t * (rr * k + n * rr + k + 2 * n)
        shape = "{}:t{}k{}n{}r{}".format(name, t, k, n, rr)
        for op, fn in (("lora_shrink_expand", ours),
                       ("lora_eager_bmm", eager)):
            dt = timeit(fn)
            results.append(dict(op=op, shape=shape, us=dt * 1e6,
                                gbps=bytes_moved / dt / 1e9))


def bench_guided(results):
    """Guided decoding sampling step (csrc/token_mask.hip), bf16 logits, a
    density-0.5 bitmask bank: the out-of-place mask and the fused mask+draw
    next to the eager torch composition of the same step (unpack bits ->
    masked_fill -> argmax / the grouped gumbel sampler), same process."""
    shifts = torch.arange(32, dtype=torch.int32, device="cuda")
    for v in (32000, 128256):
        words = (v + 31) // 32
        bank = torch.randint(-2**31, 2**31 - 1, (64, words), device="cuda",
                             dtype=torch.int32)
        if v % 32:
            bank[:, -1] &= (1 << (v % 32)) - 1
        for b in (1, 8, 64):
            logits = torch.randn(b, v, device="cuda", dtype=torch.bfloat16)
            slot = (torch.arange(b, device="cuda") % 64).to(torch.int32)
            greedy = torch.zeros(b, device="cuda")
            temp = torch.full((b,), 0.8, device="cuda")
            seed = torch.arange(b, device="cuda", dtype=torch.int32)

            def eager_mask():
                rows = bank.index_select(0, slot.long())
                bits = ((rows.unsqueeze(-1) >> shifts) & 1).view(b, -1)
                return logits.masked_fill(bits[:, :v] == 0, float("-inf"))

            cases = [
                ("guided_apply", lambda: ops.apply_token_bitmask(
                    logits, bank, slot)),
                ("guided_apply_eager", eager_mask),
                ("guided_sample_greedy", lambda: ops.sample_token_bitmask(
                    logits, bank, slot, greedy, seed)),
                ("guided_greedy_eager", lambda: eager_mask().argmax(-1)),
                ("guided_sample_fused", lambda: ops.sample_token_bitmask(
                    logits, bank, slot, temp, seed)),
                ("guided_apply+sampler", lambda: ops.sample_top_k_top_p(
                    ops.apply_token_bitmask(logits, bank, slot),
                    temperature=0.8)),
                ("guided_sample_eager", lambda: ops.sample_top_k_top_p(
                    eager_mask(), temperature=0.8)),
            ]
            # logits read (+ masked copy written by the apply variants)
            for op, fn in cases:
                dt = timeit(fn, iters=200, warmup=20)
                results.append(dict(op=op, shape="{}x{}".format(b, v),
                                    us=dt * 1e6,
                                    gbps=logits.numel() * 2 / dt / 1e9))


def bench_moe(results):
    """Mixtral-8x7B MoE layer (H 4096, I 14336, E 8, k 2), expert FFN only
    (ids/weights from a seeded randn router): the fused grouped-GEMM path
    (csrc/moe.hip) at both row-block sizes next to the eager per-expert
    hipBLASLt loop (nonzero -> linear -> silu_mul -> linear -> index_add_).
    GB/s is over the expert-weight bytes actually touched: the experts hit
    by this routing x 3*I*H bf16. For T <= 64 the fused path is also timed
    as a captured-graph replay; the eager loop reads per-expert row sets
    back to the host (nonzero), so it cannot be captured at all."""
    h, inter, e, k = 4096, 14336, 8, 2
    g = torch.Generator().manual_seed(0)
    w13 = (torch.randn(e, 2 * inter, h, generator=g) * h ** -0.5
           ).to(torch.bfloat16).cuda()
    w2 = (torch.randn(e, h, inter, generator=g) * inter ** -0.5
          ).to(torch.bfloat16).cuda()
    for t in (1, 8, 64, 128, 256, 512, 2048):
        x = torch.randn(t, h, generator=g).to(torch.bfloat16).cuda()
        ids, wts = ops.moe_route(torch.randn(t, e, generator=g).cuda(), k)
        hit = int(ids.unique().numel())
        bytes_moved = 2.0 * hit * 3 * inter * h
        shape = "t{}:experts_hit{}".format(t, hit)
        cases = [
            ("moe_fused_bm16", lambda: ops.moe_experts(
                x, w13, w2, ids, wts, block_m=16)),
            ("moe_fused_bm64", lambda: ops.moe_experts(
                x, w13, w2, ids, wts, block_m=64)),
            ("moe_eager_loop", lambda: ops._moe_experts_loop(
                x, w13, w2, ids, wts)),
        ]
        if t <= 64:
            for bm in (16, 64):
                fn = cases[0 if bm == 16 else 1][1]
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    fn()
                torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    fn()
                cases.append(("moe_fused_bm{}_graph".format(bm),
                              graph.replay))
        iters = 50 if t <= 64 else 10
        best = {}
        for _ in range(3):  # alternate the variants, keep each one's median
            for op, fn in cases:
                best.setdefault(op, []).append(
                    timeit(fn, iters=iters, warmup=5))
        for op, _fn in cases:
            dt = sorted(best[op])[1]
            results.append(dict(op=op, shape=shape, us=dt * 1e6,
                                gbps=bytes_moved / dt / 1e9))


BENCHES = {"attention": bench_attention, "decode": bench_decode,
           "memops": bench_memops, "gemm": bench_gemm,
           "sampling": bench_sampling, "lora": bench_lora,
           "guided": bench_guided, "moe": bench_moe}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--only", type=str, default=None, choices=sorted(BENCHES),
                    help="run one entry instead of all")
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.has_extension()
    results = []
    for name, fn in BENCHES.items():
        if args.only in (None, name):
            fn(results)
    for r in results:
        perf = ("{:8.1f} TF".format(r["tflops"]) if "tflops" in r
                else "{:8.1f} GB/s".format(r["gbps"]))
        print("{:28s} {:22s} {:9.1f} us {}".format(
            r["op"], r["shape"], r["us"], perf))
    if args.out:
        with open(args.out, "wt") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
