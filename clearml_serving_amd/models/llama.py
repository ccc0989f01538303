"""Llama-family decoder for the native LLM engine.

Llama-3 architecture (RMSNorm, SwiGLU MLP, RoPE, GQA) built directly on the
HIP op library with a paged KV cache (the reference delegates all of this to
vLLM, preprocess_service.py:619-1095):

- prefill: padded [B, S] token batch; fused causal flash attention with
  per-sequence lengths; computed K/V scattered into cache pages
  (ops.kv_cache_write) so decode continues where prefill left off
- decode:  [B] one-token batch; paged decode attention (ops.attention_decode)
- RMSNorm keeps the residual stream in place (one HBM pass per norm);
  SwiGLU uses the fused silu_mul kernel; QKV and gate+up are single merged
  GEMMs (hipBLASLt)

Presets: llama-3-8b (the BASELINE.json TP=8 target), plus scaled-down
variants for tests.
"""

import math
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from .. import ops
from . import register_arch
from .rope_scaling import rope_inv_freq


@dataclass
class LlamaConfig:
    vocab_size: int = 128256
    hidden: int = 4096
    layers: int = 32
    heads: int = 32
    kv_heads: int = 8
    intermediate: int = 14336
    rope_theta: float = 500000.0
    rms_eps: float = 1e-5
    max_position: int = 8192
    tie_embeddings: bool = False
    qkv_bias: bool = False  # Qwen2-family checkpoints carry QKV biases
    # mixture of experts (Mixtral): 0 = dense MLP. With experts the MLP is a
    # router + top-k routed SwiGLU experts (ops.moe_route / ops.moe_experts)
    num_experts: int = 0
    experts_per_tok: int = 2
    norm_topk_prob: bool = True  # renormalize the k routing weights
    # sliding-window attention (Mistral): position i sees keys j with
    # i - sliding_window < j <= i; 0 = full context
    sliding_window: int = 0
    # HuggingFace rope_scaling / rope_parameters dict (linear, llama3, yarn;
    # models/rope_scaling.py). None = plain RoPE from rope_theta
    rope_scaling: Optional[dict] = None
    # Qwen3: per-head RMSNorm on q and k before RoPE
    qk_norm: bool = False
    # head size when it is not hidden // heads (Qwen3-0.6B: 1024 / 16 heads
    # with head_dim 128); 0 = derived
    head_dim_override: int = 0

    @property
    def head_dim(self) -> int:
        return self.head_dim_override or self.hidden // self.heads

    @property
    def fused_qk_rope(self) -> bool:
        """Scaled RoPE and the q/k norm run in ops.qk_rope_kv; every other
        config keeps rope_inplace + kv_cache_write."""
        return bool(self.rope_scaling) or self.qk_norm


def verify_attn_supported(seq: int, heads: int, kv_heads: int,
                          head_dim: int) -> bool:
    """Shapes ops.attention_decode_multi serves (attention_verify.hip): up
    to 8 query tokens per sequence, GQA group up to 8, head_dim 64 or 128.
    Anything else (num_spec_tokens above 7, say) keeps the chunk kernel."""
    return (1 <= seq <= ops.DECODE_MULTI_MAX_Q
            and heads % kv_heads == 0
            and heads // kv_heads <= ops.DECODE_MULTI_MAX_GQ
            and head_dim in (64, 128))


class LlamaLayer(nn.Module):
    def __init__(self, cfg: LlamaConfig, tp_rank: int = 0, tp_size: int = 1,
                 layer_idx: int = 0):
        super().__init__()
        self.cfg = cfg
        self.layer_idx = layer_idx  # this layer's slice of a LoraBank
        assert cfg.heads % tp_size == 0 and cfg.kv_heads % tp_size == 0, \
            "TP degree must divide head counts"
        self.heads = cfg.heads // tp_size
        self.kv_heads = cfg.kv_heads // tp_size
        self.head_dim = cfg.head_dim
        self.tp_size = tp_size
        h, hd = cfg.hidden, cfg.head_dim
        q_out = self.heads * hd
        kv_out = self.kv_heads * hd
        inter = cfg.intermediate // tp_size

        self.attn_norm = nn.Parameter(torch.ones(h))
        self.qkv = nn.Linear(h, q_out + 2 * kv_out, bias=cfg.qkv_bias)
        self.o_proj = nn.Linear(q_out, h, bias=False)
        self.mlp_norm = nn.Parameter(torch.ones(h))
        if cfg.num_experts > 0:
            assert tp_size == 1, "experts are not sharded: MoE serves at tp=1"
            # expert stacks in the layout the grouped GEMMs stream: w13[e]
            # is gate rows then up rows, both [out, in] like nn.Linear
            self.router = nn.Linear(h, cfg.num_experts, bias=False)
            self.w13 = nn.Parameter(
                torch.empty(cfg.num_experts, 2 * inter, h))
            self.w2 = nn.Parameter(torch.empty(cfg.num_experts, h, inter))
        else:
            self.gate_up = nn.Linear(h, 2 * inter, bias=False)
            self.down = nn.Linear(inter, h, bias=False)
        self.inter = inter
        # q/k norm weights cover one head, so they replicate under TP
        if cfg.qk_norm:
            self.q_norm = nn.Parameter(torch.ones(hd))
            self.k_norm = nn.Parameter(torch.ones(hd))
        else:
            self.q_norm = self.k_norm = None
        self._inv_freq_f32, self.attn_factor = None, 1.0
        if cfg.fused_qk_rope:
            self._inv_freq_f32, self.attn_factor = rope_inv_freq(
                hd, cfg.rope_theta, cfg.rope_scaling, cfg.max_position)
            self.register_buffer("inv_freq", self._inv_freq_f32.clone(),
                                 persistent=False)

    def _apply(self, fn, recurse=True):
        # model.to(bf16) casts floating buffers; the frequency table must
        # stay exact float32, so it is restored from the host copy
        super()._apply(fn, recurse)
        if self._inv_freq_f32 is not None:
            self.inv_freq = self._inv_freq_f32.to(self.inv_freq.device)
        return self

    @staticmethod
    def _proj(mod, x):
        # decode-shaped rows route to the in-tree skinny MFMA kernel;
        # prefill rows and non-plain modules (e.g. Fp8Linear) fall through
        if type(mod) is nn.Linear:
            y = ops.skinny_linear(x, mod.weight)
            if mod.bias is not None:  # Qwen2 QKV bias (skinny kernel is
                y = y + mod.bias      # bias-free; one fused add per call)
            return y
        return mod(x)

    def _lora(self, proj, x, out, lora):
        """Add the per-token adapter delta to a projection output in place
        (multi-LoRA serving, models/lora.py): lora = (bank, idx int32 [T]),
        rows with idx -1 keep the base output bit-identical."""
        bank, idx = lora
        a, b = bank.layer(self.layer_idx, proj)
        ops.lora_expand_add(ops.lora_shrink(x, a, idx), b, idx, out)

    def forward(self, x, residual, positions, kv_cache, attn_ctx):
        attn_out = self.attn_half(x, residual, positions, kv_cache, attn_ctx)
        if self.tp_size > 1:
            from ..parallel import tp as tp_mod

            tp_mod.maybe_all_reduce(attn_out)  # row-parallel o_proj
        mlp_out = self.mlp_half(attn_out, residual, attn_ctx.get("lora"))
        if self.tp_size > 1:
            from ..parallel import tp as tp_mod

            tp_mod.maybe_all_reduce(mlp_out)  # row-parallel down projection
        return mlp_out  # residual carries the stream

    def attn_half(self, x, residual, positions, kv_cache, attn_ctx):
        """norm -> qkv -> rope -> KV write -> attention -> o_proj, WITHOUT
        the row-parallel all-reduce -- the TP decode microbatch pipeline
        (LlamaForCausalLM.forward_pipelined) issues that reduce async so it
        overlaps the other microbatch's compute."""
        cfg = self.cfg
        # optional (LoraBank, idx [T]) entry: absent -> the base path below
        lora = attn_ctx.get("lora")
        # fp8 serving path (models/quant.py): activation quantization is
        # FUSED into the producing kernels -- rmsnorm/silu_mul emit fp8
        # bytes + per-row scales in the same HBM pass
        fp8 = not isinstance(self.qkv, nn.Linear)
        if fp8:
            x8, xs = ops.rmsnorm_fp8(x, self.attn_norm, cfg.rms_eps,
                                     residual=residual)
            t = x8.shape[0]
            qkv = self.qkv.forward_q(x8, xs)
        else:
            # fused: residual += x_prev; x = rmsnorm(residual)
            x = ops.rmsnorm(x, self.attn_norm, cfg.rms_eps, residual=residual)
            t = x.shape[0]
            qkv = self._proj(self.qkv, x)
            if lora is not None:  # after the Qwen2 bias add in _proj
                self._lora("qkv", x, qkv, lora)
        # token-strided views into the merged projection -- the rope /
        # kv_cache_write / decode-attention kernels are stride-aware, so no
        # .contiguous() copies on the decode hot path
        q, k, v = qkv.split(
            [self.heads * self.head_dim, self.kv_heads * self.head_dim,
             self.kv_heads * self.head_dim], dim=-1)
        q = q.unflatten(-1, (self.heads, self.head_dim))
        k = k.unflatten(-1, (self.kv_heads, self.head_dim))
        v = v.unflatten(-1, (self.kv_heads, self.head_dim))
        k_cache = v_cache = k_sc = v_sc = slots = None
        if kv_cache is not None:
            # 2-tuple (k, v) bf16 cache, or 4-tuple (k8, v8, k_scale,
            # v_scale) fp8 cache (engine cfg kv_dtype="fp8"): e4m3 bytes +
            # per-token-per-head scales, halving KV reads on long decodes
            k_cache, v_cache = kv_cache[0], kv_cache[1]
            k_sc = kv_cache[2] if len(kv_cache) > 2 else None
            v_sc = kv_cache[3] if len(kv_cache) > 2 else None
            slots = attn_ctx["slot_mapping"]
        if cfg.fused_qk_rope:
            # q/k norm + table-driven RoPE + KV write in one launch
            q, k = ops.qk_rope_kv(q, k, v, positions, self.inv_freq,
                                  self.attn_factor, self.q_norm, self.k_norm,
                                  cfg.rms_eps, k_cache, v_cache, slots, k_sc,
                                  v_sc)
        else:
            q, k = ops.rope_inplace(q, k, positions, theta=cfg.rope_theta)
            if kv_cache is not None:
                ops.kv_cache_write(k, v, k_cache, v_cache, slots, k_sc, v_sc)

        scale = 1.0 / math.sqrt(self.head_dim)
        window = cfg.sliding_window  # model constant, same on every rank
        if attn_ctx["mode"] == "prefill":
            b, s = attn_ctx["batch"], attn_ctx["seq"]
            qb = q.unflatten(0, (b, s))  # [B, S, H, D] strided views
            kb = k.unflatten(0, (b, s))
            vb = v.unflatten(0, (b, s))
            ctx = ops.attention(qb, kb, vb, causal=True, scale=scale,
                                seq_lens=attn_ctx["seq_lens"], layout="bshd",
                                window=window)
            ctx = ctx.reshape(t, self.heads * self.head_dim)
        elif attn_ctx["mode"] == "prefill_paged":
            # chunked prefill: this chunk's queries attend to the full paged
            # history (K/V of the chunk were just scattered into the cache)
            b, s = attn_ctx["batch"], attn_ctx["seq"]
            # speculative verification (engine sets "verify"): a few query
            # tokens per sequence take the split-KV multi-query kernel;
            # chunked prefill and unsupported shapes keep the chunk kernel
            attend = ops.attention_prefill_paged
            if attn_ctx.get("verify") and verify_attn_supported(
                    s, self.heads, self.kv_heads, self.head_dim):
                attend = ops.attention_decode_multi
                attn_ctx["verify_multi"] = True  # engine stats
            ctx = attend(
                q.unflatten(0, (b, s)), k_cache, v_cache,
                attn_ctx["block_table"], attn_ctx["kv_lens"],
                attn_ctx["q_lens"], scale=scale, k_scale=k_sc, v_scale=v_sc,
                window=window)
            ctx = ctx.reshape(t, self.heads * self.head_dim)
        else:  # decode: one token per sequence
            ctx = ops.attention_decode(
                q, k_cache, v_cache, attn_ctx["block_table"],
                attn_ctx["seq_lens"], scale=scale, k_scale=k_sc, v_scale=v_sc,
                window=window)
            ctx = ctx.view(t, self.heads * self.head_dim)
        if fp8:
            # attention context has no fused producer: one-pass dynamic quant
            c8, cs = ops.quant_fp8(ctx)
            attn_out = self.o_proj.forward_q(c8, cs)
        else:
            attn_out = self._proj(self.o_proj, ctx)
            if lora is not None:
                self._lora("o_proj", ctx, attn_out, lora)
        return attn_out

    def mlp_half(self, attn_out, residual, lora=None):
        """norm -> gate_up -> silu*up -> down, WITHOUT the row-parallel
        all-reduce (see attn_half). ``lora``: attn_ctx["lora"] or None."""
        cfg = self.cfg
        if cfg.num_experts > 0 and getattr(self, "w13_e8", None) is not None:
            # MXFP4 experts (models/quant.py): the fp8 data flow below with
            # the tiled e2m1 stacks; w13 / w2 are uint8 here too, so the
            # e8m0 scale buffer is what tells the two apart
            x8, xs = ops.rmsnorm_fp8(attn_out, self.mlp_norm, cfg.rms_eps,
                                     residual=residual)
            dt = attn_out.dtype
            x = x8.view(torch.float8_e4m3fn).to(dt) * xs.to(dt)[:, None]
            ids, weights = ops.moe_route(self.router(x), cfg.experts_per_tok,
                                         cfg.norm_topk_prob)
            out = ops.moe_experts_mxfp4(
                x8, xs, self.w13, self.w13_e8, self.w13_scale, self.w2,
                self.w2_e8, self.w2_scale, ids, weights)
            return out if out.dtype == dt else out.to(dt)
        if cfg.num_experts > 0 and self.w13.dtype == torch.uint8:
            # fp8 experts (models/quant.py): the norm emits the e4m3 row and
            # its scale in one pass; the router runs on that row dequantised
            # once in the model dtype, so routing sees what the experts see
            x8, xs = ops.rmsnorm_fp8(attn_out, self.mlp_norm, cfg.rms_eps,
                                     residual=residual)
            dt = attn_out.dtype
            x = x8.view(torch.float8_e4m3fn).to(dt) * xs.to(dt)[:, None]
            ids, weights = ops.moe_route(self.router(x), cfg.experts_per_tok,
                                         cfg.norm_topk_prob)
            out = ops.moe_experts_fp8(x8, xs, self.w13, self.w13_scale,
                                      self.w2, self.w2_scale, ids, weights)
            return out if out.dtype == dt else out.to(dt)
        if cfg.num_experts > 0:
            # norm -> router -> routed experts; every launch is sync-free,
            # so the block captures into the decode graphs
            x = ops.rmsnorm(attn_out, self.mlp_norm, cfg.rms_eps,
                            residual=residual)
            ids, weights = ops.moe_route(self.router(x), cfg.experts_per_tok,
                                         cfg.norm_topk_prob)
            return ops.moe_experts(x, self.w13, self.w2, ids, weights)
        fp8 = not isinstance(self.qkv, nn.Linear)
        if fp8:
            x8, xs = ops.rmsnorm_fp8(attn_out, self.mlp_norm, cfg.rms_eps,
                                     residual=residual)
            gate_up = self.gate_up.forward_q(x8, xs)
            gate, up = gate_up.split([self.inter, self.inter], dim=-1)
            g8, gs = ops.silu_mul_fp8(gate, up)
            mlp_out = self.down.forward_q(g8, gs)
        else:
            x = ops.rmsnorm(attn_out, self.mlp_norm, cfg.rms_eps,
                            residual=residual)
            gate_up = self.gate_up(x)
            if lora is not None:
                self._lora("gate_up", x, gate_up, lora)
            gate, up = gate_up.split([self.inter, self.inter], dim=-1)
            act = ops.silu_mul(gate, up)
            mlp_out = self._proj(self.down, act)
            if lora is not None:
                self._lora("down", act, mlp_out, lora)
        return mlp_out


class LlamaForCausalLM(nn.Module):
    def __init__(self, cfg: LlamaConfig, tp_rank: int = 0, tp_size: int = 1):
        super().__init__()
        self.cfg = cfg
        self.tp_rank, self.tp_size = tp_rank, tp_size
        self.embed = nn.Embedding(cfg.vocab_size, cfg.hidden)
        self.layers = nn.ModuleList(
            [LlamaLayer(cfg, tp_rank, tp_size, layer_idx=i)
             for i in range(cfg.layers)])
        self.final_norm = nn.Parameter(torch.ones(cfg.hidden))
        # TP: lm_head column-parallel over vocab (shards all-gathered)
        assert cfg.vocab_size % tp_size == 0
        self.lm_head = nn.Linear(cfg.hidden, cfg.vocab_size // tp_size,
                                 bias=False)
        if cfg.tie_embeddings and tp_size == 1:
            self.lm_head.weight = self.embed.weight
        self._init_weights()

    def _init_weights(self):
        std = 0.02
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, std=std)
            elif isinstance(m, nn.Embedding):
                nn.init.normal_(m.weight, std=std)
        # expert stacks are bare Parameters, which modules() does not visit;
        # drawn after the loop, so dense models consume the RNG as before
        for layer in self.layers:
            if self.cfg.num_experts > 0:
                nn.init.normal_(layer.w13, std=std)
                nn.init.normal_(layer.w2, std=std)

    def forward(
        self,
        tokens: torch.Tensor,      # [T] flat token ids
        positions: torch.Tensor,   # [T] int32
        kv_caches: Optional[List] = None,  # per layer (k_cache, v_cache)
        attn_ctx: Optional[Dict] = None,
        last_token_idx: Optional[torch.Tensor] = None,
        return_hidden: bool = False,
        gather_logits: bool = True,
    ) -> torch.Tensor:
        """Returns logits [n_seqs, vocab] at the selected token positions
        (or the final-norm hidden states [T, hidden] when ``return_hidden``
        -- the embeddings serve path)."""
        x = self.embed(tokens.long())
        residual = torch.zeros_like(x)
        for i, layer in enumerate(self.layers):
            cache = kv_caches[i] if kv_caches is not None else None
            x = layer(x, residual, positions, cache, attn_ctx)
        x = ops.rmsnorm(x, self.final_norm, self.cfg.rms_eps,
                        residual=residual)
        if last_token_idx is not None:
            x = x[last_token_idx.long()]
        if return_hidden:
            return x
        logits = self.lm_head(x)
        if self.tp_size > 1 and gather_logits:
            return self._gathered(logits)
        return logits

    def _gathered(self, logits):
        # lm_head is column-sharded. The serving engine passes
        # gather_logits=False and samples ON the shards (packed-argmax /
        # Gumbel-max all-reduce of O(batch) words, parallel/tp.py) --
        # the full-vocab all-gather (b x 128k x 2B per decode step) is
        # only for offline full-logits consumers like the TP math tests.
        from ..parallel import tp as tp_mod

        return tp_mod.gather_logits(logits)

    def forward_pipelined(self, parts, kv_caches):
        """TP decode comm/compute overlap: run N microbatches through the
        layer stack in a 2-stage pipeline -- each half's row-parallel
        all-reduce is issued async and waited only when ITS next consumer
        runs, so the collective overlaps the other half's GEMMs (xGMI comm
        under compute; ROADMAP 'decode microbatch pipelining').

        parts: list of (tokens, positions, attn_ctx); returns concatenated
        logits rows in part order (gather_logits=False semantics). Issue
        order per layer is identical on every rank (attn_0, attn_1, mlp_0,
        mlp_1), so the collectives line up."""
        from ..parallel import tp as tp_mod

        n = len(parts)
        xs, residuals = [], []
        for tokens, positions, _ctx in parts:
            x = self.embed(tokens.long())
            residuals.append(torch.zeros_like(x))
            xs.append(x)
        works = [None] * n
        for li, layer in enumerate(self.layers):
            cache = kv_caches[li] if kv_caches is not None else None
            attn = [None] * n
            for j in range(n):
                if works[j] is not None:
                    works[j].wait()  # previous mlp reduce of THIS half
                attn[j] = layer.attn_half(xs[j], residuals[j], parts[j][1],
                                          cache, parts[j][2])
                works[j] = tp_mod.all_reduce_async(attn[j])
            for j in range(n):
                if works[j] is not None:
                    works[j].wait()  # attn reduce of this half
                xs[j] = layer.mlp_half(attn[j], residuals[j])
                works[j] = tp_mod.all_reduce_async(xs[j])
        outs = []
        for j in range(n):
            if works[j] is not None:
                works[j].wait()
            h = ops.rmsnorm(xs[j], self.final_norm, self.cfg.rms_eps,
                            residual=residuals[j])
            outs.append(self.lm_head(h))
        return torch.cat(outs, dim=0)


PRESETS = {
    "llama-3-8b": LlamaConfig(),
    "llama-3-1b": LlamaConfig(hidden=2048, layers=16, heads=32, kv_heads=8,
                              intermediate=8192, tie_embeddings=True),
    "llama-tiny": LlamaConfig(vocab_size=512, hidden=256, layers=2, heads=4,
                              kv_heads=2, intermediate=512, rope_theta=10000.0,
                              max_position=512),
    # Qwen2 family: llama architecture + QKV biases + ChatML template
    # (models/convert.py convert_hf_qwen2; numerics pinned vs transformers
    # in tests/test_hf_convert.py)
    "qwen2-7b": LlamaConfig(vocab_size=152064, hidden=3584, layers=28,
                            heads=28, kv_heads=4, intermediate=18944,
                            rope_theta=1e6, rms_eps=1e-6, max_position=32768,
                            qkv_bias=True),
    "qwen2-1.5b": LlamaConfig(vocab_size=151936, hidden=1536, layers=28,
                              heads=12, kv_heads=2, intermediate=8960,
                              rope_theta=1e6, rms_eps=1e-6,
                              max_position=32768, qkv_bias=True,
                              tie_embeddings=True),
    # Mixtral: llama attention + 8 SwiGLU experts, top-2 routing
    # (models/convert.py convert_hf_mixtral; numerics pinned vs transformers
    # in tests/test_moe_cpu.py). 8x7B is ~93 GB in bf16: one MI355X.
    "mixtral-8x7b": LlamaConfig(vocab_size=32000, hidden=4096, layers=32,
                                heads=32, kv_heads=8, intermediate=14336,
                                rope_theta=1e6, rms_eps=1e-5,
                                max_position=32768, num_experts=8,
                                experts_per_tok=2),
    "mixtral-tiny": LlamaConfig(vocab_size=512, hidden=256, layers=2, heads=4,
                                kv_heads=2, intermediate=512,
                                rope_theta=10000.0, max_position=512,
                                num_experts=4, experts_per_tok=2),
    # Mistral-7B-v0.1: llama tensor names (convert_hf_llama) + a 4096-key
    # sliding window (numerics pinned vs transformers in
    # tests/test_sliding_window_cpu.py)
    "mistral-7b": LlamaConfig(vocab_size=32000, hidden=4096, layers=32,
                              heads=32, kv_heads=8, intermediate=14336,
                              rope_theta=10000.0, rms_eps=1e-5,
                              max_position=32768, sliding_window=4096),
    # window 24 on purpose: the default 16-token KV page does not divide it
    "mistral-tiny": LlamaConfig(vocab_size=512, hidden=256, layers=2, heads=4,
                                kv_heads=2, intermediate=512,
                                rope_theta=10000.0, max_position=512,
                                sliding_window=24),
    # Llama-3.1 / 3.2: Llama-3 + rope_scaling "llama3". Qwen3 (dense): q/k
    # norm, no QKV bias, head_dim a field of its own. The full-size numbers
    # below could not be checked against the hub from here; real checkpoints
    # take their shape from config.json (models/convert.py
    # llama_config_from_hf). Numerics pinned vs transformers in
    # tests/test_qwen3_llama31_cpu.py.
    "llama-3.1-8b": LlamaConfig(max_position=131072, rope_scaling={
        "rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0,
        "high_freq_factor": 4.0, "original_max_position_embeddings": 8192}),
    "llama-3.2-1b": LlamaConfig(
        hidden=2048, layers=16, heads=32, kv_heads=8, intermediate=8192,
        tie_embeddings=True, max_position=131072, rope_scaling={
            "rope_type": "llama3", "factor": 32.0, "low_freq_factor": 1.0,
            "high_freq_factor": 4.0,
            "original_max_position_embeddings": 8192}),
    "qwen3-8b": LlamaConfig(vocab_size=151936, hidden=4096, layers=36,
                            heads=32, kv_heads=8, intermediate=12288,
                            rope_theta=1e6, rms_eps=1e-6, max_position=40960,
                            qk_norm=True, head_dim_override=128),
    "qwen3-0.6b": LlamaConfig(vocab_size=151936, hidden=1024, layers=28,
                              heads=16, kv_heads=8, intermediate=3072,
                              rope_theta=1e6, rms_eps=1e-6,
                              max_position=40960, tie_embeddings=True,
                              qk_norm=True, head_dim_override=128),
    # original max 32 with factor 8: positions >= 32 reach all three bands
    "llama-3.1-tiny": LlamaConfig(
        vocab_size=512, hidden=256, layers=2, heads=4, kv_heads=2,
        intermediate=512, rope_theta=10000.0, max_position=512,
        rope_scaling={"rope_type": "llama3", "factor": 8.0,
                      "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                      "original_max_position_embeddings": 32}),
    # head_dim 128 with hidden 256 / 4 heads: the override is exercised
    "qwen3-tiny": LlamaConfig(vocab_size=512, hidden=256, layers=2, heads=4,
                              kv_heads=2, intermediate=512, rope_theta=1e6,
                              rms_eps=1e-6, max_position=512, qk_norm=True,
                              head_dim_override=128),
}


@register_arch("llama")
def llama(preset: str = "llama-3-8b", **overrides) -> LlamaForCausalLM:
    cfg_base = PRESETS[preset]
    cfg = LlamaConfig(**{**cfg_base.__dict__, **overrides})
    return LlamaForCausalLM(cfg)
