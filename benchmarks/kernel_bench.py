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
    back to the host (nonzero), so it cannot be captured at all. The same
    weights quantised to e4m3 give the fp8 rows: ops.moe_experts_fp8 fused at
    both row blocks and its per-expert scaled_mm loop; quantised to MXFP4
    (csrc/moe_mxfp4.hip, 0.53125 bytes per weight: e2m1 + an e8m0 scale per
    32) they give the mxfp4 rows: ops.moe_experts_mxfp4 fused at both row
    blocks and its per-expert dequant + bf16 matmul loop, and
    moe_mxfp4_tiled, the 128-row tiled kernels of csrc/moe_mxfp4_gemm.hip
    (block_m=128), with the fraction of the 5.03 PF e4m3 x e2m1 peak that
    its 2 * T*k * 3*I*H flop reach. Every fused row is also timed as a graph
    replay at T <= 64. T = 4096 and 8192 leave out the bf16 and fp8 fused
    rows (decode-shaped kernels, seconds per call there)."""
    h, inter, e, k = 4096, 14336, 8, 2
    g = torch.Generator().manual_seed(0)
    w13 = (torch.randn(e, 2 * inter, h, generator=g) * h ** -0.5
           ).to(torch.bfloat16).cuda()
    w2 = (torch.randn(e, h, inter, generator=g) * inter ** -0.5
          ).to(torch.bfloat16).cuda()
    # fp8 experts (csrc/moe_fp8.hip) on the same weights and routing; their
    # GB/s counts one byte per weight
    from clearml_serving_amd.models.quant import quantize_experts_fp8

    f8 = quantize_experts_fp8(w13) + quantize_experts_fp8(w2)
    from clearml_serving_amd.models.quant import quantize_experts_mxfp4

    mx = quantize_experts_mxfp4(w13) + quantize_experts_mxfp4(w2)
    for t in (1, 8, 32, 64, 128, 256, 512, 2048, 4096, 8192):
        x = torch.randn(t, h, generator=g).to(torch.bfloat16).cuda()
        ids, wts = ops.moe_route(torch.randn(t, e, generator=g).cuda(), k)
        hit = int(ids.unique().numel())
        bytes_moved = 2.0 * hit * 3 * inter * h
        shape = "t{}:experts_hit{}".format(t, hit)
        x8, xs = ops.quant_fp8(x)
        cases = [
            ("moe_fused_bm16", lambda: ops.moe_experts(
                x, w13, w2, ids, wts, block_m=16)),
            ("moe_fused_bm64", lambda: ops.moe_experts(
                x, w13, w2, ids, wts, block_m=64)),
            ("moe_eager_loop", lambda: ops._moe_experts_loop(
                x, w13, w2, ids, wts)),
            ("moe_fp8_fused_bm16", lambda: ops.moe_experts_fp8(
                x8, xs, *f8, ids, wts, block_m=16)),
            ("moe_fp8_fused_bm64", lambda: ops.moe_experts_fp8(
                x8, xs, *f8, ids, wts, block_m=64)),
            ("moe_fp8_loop", lambda: ops._moe_experts_fp8_loop(
                x8, xs, *f8, ids, wts)),
            ("moe_mxfp4_fused_bm16", lambda: ops.moe_experts_mxfp4(
                x8, xs, *mx, ids, wts, block_m=16)),
            ("moe_mxfp4_fused_bm64", lambda: ops.moe_experts_mxfp4(
                x8, xs, *mx, ids, wts, block_m=64)),
            ("moe_mxfp4_loop", lambda: ops._moe_experts_mxfp4_loop(
                x8, xs, *mx, ids, wts)),
            ("moe_mxfp4_tiled", lambda: ops.moe_experts_mxfp4(
                x8, xs, *mx, ids, wts, block_m=128)),
        ]
        if t > 2048:
            cases = [c for c in cases
                     if "mxfp4" in c[0] or c[0].endswith("_loop")]
        if t <= 64:
            for op, fn in [c for c in cases if "fused" in c[0]]:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    fn()
                torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    fn()
                cases.append((op + "_graph", graph.replay))
        iters = 50 if t <= 64 else 10
        best = {}
        for _ in range(3):  # alternate the variants, keep each one's median
            for op, fn in cases:
                best.setdefault(op, []).append(
                    timeit(fn, iters=iters, warmup=5))
        for op, _fn in cases:
            dt = sorted(best[op])[1]
            nbytes = (bytes_moved / 2 if "fp8" in op
                      else bytes_moved / 2 * 0.53125 if "mxfp4" in op
                      else bytes_moved)
            results.append(dict(op=op, shape=shape, us=dt * 1e6,
                                gbps=nbytes / dt / 1e9))
            if op == "moe_mxfp4_tiled":
                flops = 2.0 * t * k * 3 * inter * h
                results[-1]["shape"] += " {:.1%} of MX-peak".format(
                    flops / dt / 5.03e15)


def bench_sample_rows(results):
    """Fused per-row sampler and penalties (csrc/sample_rows.hip), bf16
    logits, V = 128256, old and new paths alternated in one process (median
    of three): top-k 50 / top-p 0.9 on every row against the library
    composition of sample_top_k_top_p; plain rows against
    sample_token_bitmask at slot -1; apply_penalties with 512 entries per
    row against clone + per-row index updates. "filters_off" passes the
    filter tensors with every row's filter off (the select kernel launches
    and leaves at once), which is what plain rows pay inside a mixed engine
    batch. At B = 64 the batch is also run with 64 distinct (top_k, top_p)
    settings: 64 grouped calls with a copy back each, as the engine's
    grouped path issues them, against one sample_rows call and one copy.
    GB/s (logits read once) is given for the plain single-pass rows only."""
    v, ext = 128256, ops.extension_or_none()
    bank = torch.zeros(1, (v + 31) // 32, dtype=torch.int32, device="cuda")
    for b in (1, 8, 64):
        logits = (torch.randn(b, v, device="cuda") * 3).to(torch.bfloat16)
        temp = torch.full((b,), 0.8, device="cuda")
        seed = torch.arange(b, device="cuda", dtype=torch.int32)
        k = torch.full((b,), 50, device="cuda", dtype=torch.int32)
        p = torch.full((b,), 0.9, device="cuda")
        k_off, p_off, m_off = k * 0, p * 0 + 1, p * 0
        slot = torch.full((b,), -1, device="cuda", dtype=torch.int32)
        n = 512
        tok = torch.stack([torch.randperm(v, device="cuda")[:n]
                           for _ in range(b)]).to(torch.int32)
        cnt = torch.randint(0, 3, (b * n,), device="cuda", dtype=torch.int32)
        flags = torch.zeros(b * n, device="cuda", dtype=torch.int32)
        offs = torch.arange(b + 1, device="cuda", dtype=torch.int32) * n
        pres = torch.full((b,), 0.5, device="cuda")
        freq = torch.full((b,), 0.2, device="cuda")
        rep = torch.full((b,), 1.2, device="cuda")

        def penalties_eager():
            out = logits.clone()
            for r in range(b):
                idx = tok[r].long()
                c = cnt[r * n:(r + 1) * n].float()
                x = out[r, idx].float()
                x = torch.where(x > 0, x / 1.2, x * 1.2) - 0.2 * c
                out[r, idx] = (x - 0.5 * (c > 0)).to(out.dtype)
            return out

        cases = [
            ("sampler_k50_p0.9_library", lambda: ext.sample_top_k_top_p(
                logits, 0.8, 50, 0.9, 7)),
            ("sampler_k50_p0.9_sample_rows", lambda: ops.sample_rows(
                logits, temp, k, p, None, seed)),
            ("sampler_plain_token_bitmask", lambda: ops.sample_token_bitmask(
                logits, bank, slot, temp, seed)),
            ("sampler_plain_sample_rows", lambda: ops.sample_rows(
                logits, temp, None, None, None, seed)),
            ("sampler_plain_filters_off", lambda: ops.sample_rows(
                logits, temp, k_off, p_off, m_off, seed)),
            ("penalties_eager_rows", penalties_eager),
            ("penalties_apply_penalties", lambda: ops.apply_penalties(
                logits, tok.view(-1), cnt, flags, offs, pres, freq, rep)),
        ]
        if b == 64:
            ks = [20 + r for r in range(b)]
            ps = [0.5 + 0.007 * r for r in range(b)]
            kd = torch.tensor(ks, device="cuda", dtype=torch.int32)
            pd = torch.tensor(ps, device="cuda")
            cases += [
                ("sampler_64_settings_grouped", lambda: [
                    ext.sample_top_k_top_p(logits[[r]], 0.8, ks[r], ps[r],
                                           7).cpu() for r in range(b)]),
                ("sampler_64_settings_sample_rows", lambda: ops.sample_rows(
                    logits, temp, kd, pd, None, seed).cpu()),
            ]
        runs = {}
        for _ in range(3):
            for op, fn in cases:
                runs.setdefault(op, []).append(timeit(fn, iters=100,
                                                      warmup=10))
        for op, _fn in cases:
            lo, dt, hi = sorted(runs[op])
            r = dict(op=op, shape="{}x{} [{:.1f}-{:.1f}us]".format(
                b, v, lo * 1e6, hi * 1e6), us=dt * 1e6)
            if op.startswith("sampler_plain"):
                r["gbps"] = logits.numel() * 2 / dt / 1e9
            results.append(r)


def bench_qk_rope_kv(results):
    """Fused norm-less ops.qk_rope_kv (csrc/qk_rope_kv.hip) against the
    rope_inplace + kv_cache_write pair it stands in for, Llama-3-8B head
    shapes (32 / 8 heads, D = 128), bf16 and fp8 caches, q/k/v as views of
    the merged QKV output. Each side is a captured graph of 16 repetitions
    (the ops live inside decode graphs; an eager A/B would mostly time two
    launches against one), the two graphs are replayed alternately and the
    median of three rounds is kept. us is per repetition; GB/s counts the
    bytes the stretch needs (q, k read and written, v read, both cache rows
    written) for either side."""
    hq, hkv, d, bs, reps = 32, 8, 128, 16, 16
    from clearml_serving_amd.models.rope_scaling import rope_inv_freq

    inv_freq = rope_inv_freq(d, 500000.0, None, 8192)[0].cuda()
    for t in (1, 64, 2048):
        for kv in ("bf16", "fp8"):
            qkv = torch.randn(t, (hq + 2 * hkv) * d, device="cuda",
                              dtype=torch.bfloat16)
            q, k, v = (x.unflatten(-1, (-1, d)) for x in qkv.split(
                [hq * d, hkv * d, hkv * d], dim=-1))
            pos = torch.arange(t, device="cuda", dtype=torch.int32) + 1000
            slots = torch.arange(t, device="cuda", dtype=torch.int32)
            nb = (t + bs - 1) // bs
            kc = torch.zeros(nb, hkv, bs, d, device="cuda",
                             dtype=torch.uint8 if kv == "fp8"
                             else torch.bfloat16)
            vc = torch.zeros_like(kc)
            sc = ((torch.ones(nb, hkv, bs, device="cuda"),
                   torch.ones(nb, hkv, bs, device="cuda"))
                  if kv == "fp8" else (None, None))

            def pair():
                ops.rope_inplace(q, k, pos, theta=500000.0)
                ops.kv_cache_write(k, v, kc, vc, slots, *sc)

            def fused():
                ops.qk_rope_kv(q, k, v, pos, inv_freq, 1.0, None, None, 1e-6,
                               kc, vc, slots, *sc)

            graphs = {}
            for name, fn in (("rope+kv_write", pair), ("qk_rope_kv", fused)):
                fn()
                torch.cuda.synchronize()
                graphs[name] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[name]):
                    for _ in range(reps):
                        fn()
            runs = {}
            for _ in range(3):
                for name, graph in graphs.items():
                    runs.setdefault(name, []).append(
                        timeit(graph.replay, iters=200, warmup=20) / reps)
            nbytes = t * d * (4 * (hq + hkv) + 2 * hkv
                              + 2 * hkv * kc.element_size())
            for name in graphs:
                lo, dt, hi = sorted(runs[name])
                results.append(dict(
                    op="{}_{}".format(name, kv),
                    shape="T={} [{:.2f}-{:.2f}us]".format(t, lo * 1e6,
                                                          hi * 1e6),
                    us=dt * 1e6, gbps=nbytes / dt / 1e9))


def bench_mxfp4(results):
    """ops.skinny_gemm_mxfp4 (csrc/mxfp4_path.hip, 4 and 8 k-split waves) at
    the Llama-3-8B projection shapes against ops.skinny_gemm_fp8 on the same
    weights in e4m3 and against Mxfp4Linear's dequant + bf16 matmul route.
    Decode streams every layer's weights once per step, so each side runs
    over enough clones of its weight to exceed the 256 MiB last-level cache
    (at least 8), one call per clone captured into a graph; the graphs are
    replayed alternately and the median of three rounds is kept. us is per
    call; GB/s counts the weight bytes of the side (elements + scales)."""
    from clearml_serving_amd.models.quant import F8, F8_MAX

    shapes = (("qkv", 6144, 4096), ("o_proj", 4096, 4096),
              ("gate_up", 28672, 4096), ("down", 4096, 14336))
    for name, n, k in shapes:
        w = torch.randn(n, k, device="cuda") / 32
        w4, e8, rs = ops.quantize_mxfp4(w)
        w4t, e8t = ops.tile_mxfp4_weight(w4, e8)
        ws8 = w.abs().amax(dim=1) / F8_MAX
        w8 = ops.swizzle_fp8_weight((w / ws8[:, None]).to(F8).view(torch.uint8))
        del w, w4, e8
        mx_bytes, f8_bytes = w4t.numel() + e8t.numel(), w8.numel()
        mx = [(w4t.clone(), e8t.clone())
              for _ in range(max(8, -(-(300 << 20) // mx_bytes)))]
        f8 = [w8.clone() for _ in range(max(8, -(-(300 << 20) // f8_bytes)))]
        for m in (1, 8, 16, 32, 64):
            x8, xs = ops.quant_fp8(torch.randn(m, k, device="cuda",
                                               dtype=torch.bfloat16))

            def dequant_route(wt, et):
                wd = ops.dequant_mxfp4_bf16(wt, et, rs, n, k)
                return (x8.view(F8).to(torch.bfloat16) @ wd.t()).float() \
                    * xs[:, None]

            sides = {
                "mxfp4_w4": lambda: [ops.skinny_gemm_mxfp4(
                    x8, xs, wt, et, rs, waves=4) for wt, et in mx],
                "mxfp4_w8": lambda: [ops.skinny_gemm_mxfp4(
                    x8, xs, wt, et, rs, waves=8) for wt, et in mx],
                "fp8_skinny": lambda: [ops.skinny_gemm_fp8(
                    x8, xs, wq, ws8, swizzled=True) for wq in f8],
                "mxfp4_dequant+mm": lambda: [dequant_route(wt, et)
                                             for wt, et in mx[:8]],
            }
            calls = {"fp8_skinny": len(f8), "mxfp4_dequant+mm": 8}
            graphs = {}
            for side, fn in sides.items():
                fn()
                torch.cuda.synchronize()
                graphs[side] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[side]):
                    fn()
            runs = {}
            for _ in range(3):
                for side, graph in graphs.items():
                    runs.setdefault(side, []).append(
                        timeit(graph.replay, iters=100, warmup=5)
                        / calls.get(side, len(mx)))
            for side in graphs:
                lo, dt, hi = sorted(runs[side])
                results.append(dict(
                    op=side, shape="{} M={} [{:.1f}-{:.1f}us]".format(
                        name, m, lo * 1e6, hi * 1e6), us=dt * 1e6,
                    gbps=(f8_bytes if side == "fp8_skinny" else mx_bytes)
                    / dt / 1e9))
            del graphs


# MX matrix peak for an e4m3 x e2m1 product: v_mfma_scale_f32_16x16x128_f8f6f4
# with an 8-bit operand issues in 8 passes (32 cycles) for 2*16*16*128 FLOP,
# x 4 SIMDs x 256 CUs x 2.4 GHz = 5.03 PFLOP/s (the CDNA4 ISA guide's pass
# count; the MI355X data sheet's dense MXFP8 figure). HBM3E: 8 TB/s.
MX_PEAK_FLOPS = 2 * 16 * 16 * 128 / 32 * 4 * 256 * 2.4e9
HBM_BYTES_PER_S = 8e12


def bench_mxfp4_gemm(results):
    """ops.gemm_mxfp4 (csrc/mxfp4_gemm.hip; the default tile and both forced
    ones) at the Llama-3-8B projection shapes and prefill-sized M against
    what Mxfp4Linear.forward_q did before it: dequant_mxfp4_bf16 + bf16
    matmul + fp32 row scaling + the cast back. As bench_mxfp4: each side
    over weight clones exceeding the 256 MiB last-level cache, captured into
    its own graph, graphs replayed alternately, median of three rounds with
    min-max. us is per call; TFLOP/s from 2*M*N*K; the kernel's share of its
    bound, the larger of FLOP over the MX peak and compulsory bytes (A,
    weight tiles, C) over HBM bandwidth, with the binding one named."""
    from clearml_serving_amd.models.quant import F8

    shapes = (("qkv", 6144, 4096), ("o_proj", 4096, 4096),
              ("gate_up", 28672, 4096), ("down", 4096, 14336))
    for name, n, k in shapes:
        w4, e8, rs = ops.quantize_mxfp4(torch.randn(n, k, device="cuda") / 32)
        w4t, e8t = ops.tile_mxfp4_weight(w4, e8)
        del w4, e8
        mx_bytes = w4t.numel() + e8t.numel()
        mx = [(w4t.clone(), e8t.clone())
              for _ in range(max(8, -(-(300 << 20) // mx_bytes)))]
        for m in (128, 512, 2048, 8192):
            x8, xs = ops.quant_fp8(torch.randn(m, k, device="cuda",
                                               dtype=torch.bfloat16))

            def dequant_route(wt, et):
                wd = ops.dequant_mxfp4_bf16(wt, et, rs, n, k)
                return ((x8.view(F8).to(torch.bfloat16) @ wd.t()).float()
                        * xs[:, None]).to(torch.bfloat16)

            def tiled(tile):
                return lambda: [ops.gemm_mxfp4(x8, xs, wt, et, rs, tile=tile)
                                for wt, et in mx[:8]]

            sides = {"gemm_mxfp4": tiled(0), "gemm_mxfp4_t64": tiled(64),
                     "gemm_mxfp4_t128": tiled(128),
                     "mxfp4_dequant+mm": lambda: [dequant_route(wt, et)
                                                  for wt, et in mx[-8:]]}
            graphs, iters = {}, {}
            for side, fn in sides.items():
                fn()
                torch.cuda.synchronize()
                graphs[side] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[side]):
                    fn()
                once = timeit(graphs[side].replay, iters=2, warmup=1)
                iters[side] = int(min(100, max(3, 0.1 / once)))
            runs = {}
            for _ in range(3):
                for side, graph in graphs.items():
                    runs.setdefault(side, []).append(
                        timeit(graph.replay, iters=iters[side], warmup=2) / 8)
            flops = 2.0 * m * n * k
            t_flop = flops / MX_PEAK_FLOPS
            t_byte = (m * k + mx_bytes + 2.0 * m * n) / HBM_BYTES_PER_S
            for side in graphs:
                lo, dt, hi = sorted(runs[side])
                r = dict(op=side, shape="{} M={} [{:.1f}-{:.1f}us]".format(
                    name, m, lo * 1e6, hi * 1e6), us=dt * 1e6,
                    tflops=flops / dt / 1e12)
                if side != "mxfp4_dequant+mm":
                    r["shape"] += " {:.0%} of {} bound".format(
                        max(t_flop, t_byte) / dt,
                        "MX-peak" if t_flop >= t_byte else "HBM")
                results.append(r)
            del graphs


BENCHES = {"attention": bench_attention, "decode": bench_decode,
           "memops": bench_memops, "gemm": bench_gemm,
           "sampling": bench_sampling, "lora": bench_lora,
           "guided": bench_guided, "moe": bench_moe,
           "sample_rows": bench_sample_rows,
           "qk_rope_kv": bench_qk_rope_kv, "mxfp4": bench_mxfp4,
           "mxfp4_gemm": bench_mxfp4_gemm}


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
                else "{:8.1f} GB/s".format(r["gbps"]) if "gbps" in r else "")
        print("{:32s} {:30s} {:9.1f} us {}".format(
            r["op"], r["shape"], r["us"], perf))
    if args.out:
        with open(args.out, "wt") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
