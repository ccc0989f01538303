"""Native LLM engine: paged KV cache + continuous batching scheduler.

The in-process replacement for the reference's vLLM delegation
(preprocess_service.py:619-1095). One engine per process; requests stream
tokens through asyncio queues.

Engine step (continuous batching):
1. admit waiting prompts while the prefill-token budget and free KV blocks
   allow (prompts padded to one batch; per-seq lengths mask attention);
   with prefix caching on, a cached prompt prefix admits pre-filled
2. run ONE prefill forward for the admitted batch, scatter K/V into pages,
   sample each sequence's first token (long prompts advance in chunks,
   fair-shared, interleaving with decode)
3. run ONE decode forward for every running sequence (paged decode
   attention, hipGraph-replayed per batch bucket), sample next tokens;
   greedy sequences may take the ngram speculative path instead (several
   tokens verified in one forward, exact output)
4. emit tokens to per-request streams; finished sequences free their pages

Model families: llama / qwen2 (models/llama.py) and gpt2 (models/gpt2.py)
share one forward interface, so every scheduler feature serves both.
Opt-in subsystems, each exact by test: fp8 weights (fused activation
quant), fp8 KV cache, ngram speculation, automatic prefix caching
(content-addressed blocks, prompt + generated), TP over RCCL/xGMI with
single-tensor plan broadcast + on-shard sampling (+ opt-in microbatch
comm/compute overlap). Sampling surface: docs/API.md.

KV sizing: pages are allocated once at startup from a fraction of free HBM
(288 GB/GPU -> tens of thousands of 16-token pages for an 8B model).
"""

import asyncio
import json
import os
import random
import threading
import time
import uuid
from collections import OrderedDict, deque
from dataclasses import dataclass, field
from typing import Any, AsyncGenerator, Dict, List, Optional

import torch

from ... import ops
from ...models.llama import PRESETS, LlamaConfig, LlamaForCausalLM


# --------------------------------------------------------------------- #
# tokenizer
# --------------------------------------------------------------------- #
class SimpleTokenizer:
    """Byte-level fallback tokenizer (synthetic serving / tests: the
    environment has no model hub, so real checkpoints supply their own
    tokenizer.json)."""

    eos_id = 0
    vocab_size = 257

    def encode(self, text: str) -> List[int]:
        return [b + 1 for b in text.encode("utf-8")]

    def decode(self, ids: List[int]) -> str:
        # ids above the byte range (random-init models) fold back into it
        return bytes(min(max(0, i - 1) % 256, 255) for i in ids
                     if i > 0).decode("utf-8", errors="replace")


class HfTokenizer:
    def __init__(self, path: str):
        from tokenizers import Tokenizer

        self._tok = Tokenizer.from_file(path)
        self.vocab_size = self._tok.get_vocab_size()
        # ChatML checkpoints (Qwen2 family) carry <|im_start|>/<|im_end|>;
        # chat requests then format with ChatML and stop at <|im_end|>
        self.is_chatml = (
            self._tok.token_to_id("<|im_start|>") is not None
            and self._tok.token_to_id("<|im_end|>") is not None)
        eos = None
        cands = ("</s>", "<|eot_id|>", "<|end_of_text|>", "<|endoftext|>")
        if self.is_chatml:
            cands = ("<|im_end|>",) + cands
        for cand in cands:
            tid = self._tok.token_to_id(cand)
            if tid is not None:
                eos = tid
                break
        self.eos_id = eos if eos is not None else 0
        # llama-3 checkpoints carry header-id special tokens: chat requests
        # then format with the real llama-3 template instead of the
        # synthetic fallback (_chat_prompt)
        self.is_llama3 = (
            self._tok.token_to_id("<|start_header_id|>") is not None
            and self._tok.token_to_id("<|eot_id|>") is not None)

    def encode(self, text: str) -> List[int]:
        return self._tok.encode(text).ids

    def decode(self, ids: List[int]) -> str:
        return self._tok.decode(ids)


# --------------------------------------------------------------------- #
@dataclass
class SamplingParams:
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    max_tokens: int = 128
    stop_token_ids: List[int] = field(default_factory=list)
    stop: List[str] = field(default_factory=list)
    ignore_eos: bool = False
    seed: Optional[int] = None           # reproducible sampling per request
    presence_penalty: float = 0.0        # OpenAI: [-2, 2], output tokens
    frequency_penalty: float = 0.0       # OpenAI: [-2, 2], output counts
    repetition_penalty: float = 1.0      # CTRL-style, prompt+output tokens
    logprobs: Optional[int] = None       # None = off; N = N top_logprobs
                                         # alongside each chosen token
    min_tokens: int = 0                  # ban eos/stop-token finishes until
                                         # this many tokens are generated
    guided: Optional[tuple] = None       # (kind, spec) guided-decoding
                                         # constraint (guided.py); engines
                                         # with guided_decoding on only

    def has_penalties(self) -> bool:
        return bool(self.presence_penalty or self.frequency_penalty
                    or self.repetition_penalty != 1.0)

    @classmethod
    def from_request(cls, body: Dict[str, Any], default_max: int = 128,
                     guided: bool = False):
        """Validate at add-request time so one malformed request 422s on its
        own instead of crashing the shared step() for every in-flight
        sequence (a bad temperature would assert inside the batched
        sampling kernel)."""
        try:
            temperature = float(body.get("temperature", 1.0))
            top_k = int(body.get("top_k", 0) or 0)
            # max_completion_tokens: the newer OpenAI name for max_tokens
            top_p = float(body.get("top_p", 1.0))
            mt = body.get("max_tokens")
            if mt is None:
                mt = body.get("max_completion_tokens")
            max_tokens = int(mt) if mt is not None else int(default_max)
            def _num(key, default):
                v = body.get(key)
                return float(v) if v is not None else default

            presence = _num("presence_penalty", 0.0)
            frequency = _num("frequency_penalty", 0.0)
            repetition = _num("repetition_penalty", 1.0)
            seed = body.get("seed")
            seed = int(seed) if seed is not None else None
        except (TypeError, ValueError, OverflowError):
            raise ValueError("sampling parameters must be numeric "
                             "(temperature/top_k/top_p/max_tokens/"
                             "penalties/seed)")
        import math as _math

        if not (_math.isfinite(temperature) and temperature >= 0.0):
            raise ValueError(
                "temperature must be finite and >= 0 (0 = greedy), got "
                "{}".format(temperature))
        if top_k < 0:
            raise ValueError("top_k must be >= 0 (0 = disabled), got {}"
                             .format(top_k))
        if not (0.0 < top_p <= 1.0):
            raise ValueError("top_p must be in (0, 1], got {}".format(top_p))
        if max_tokens < 1:
            raise ValueError("max_tokens must be >= 1, got {}".format(
                max_tokens))
        try:
            min_tokens = int(body.get("min_tokens", 0) or 0)
        except (TypeError, ValueError, OverflowError):
            raise ValueError("'min_tokens' must be an int")
        if not (0 <= min_tokens <= max_tokens):
            raise ValueError(
                "min_tokens must be in [0, max_tokens], got {}".format(
                    min_tokens))
        if not (-2.0 <= presence <= 2.0):
            raise ValueError("presence_penalty must be in [-2, 2], got {}"
                             .format(presence))
        if not (-2.0 <= frequency <= 2.0):
            raise ValueError("frequency_penalty must be in [-2, 2], got {}"
                             .format(frequency))
        if not (_math.isfinite(repetition) and repetition > 0.0):
            raise ValueError("repetition_penalty must be finite and > 0, "
                             "got {}".format(repetition))
        # logprobs: completions style ("logprobs": N) or chat style
        # ("logprobs": true + "top_logprobs": N)
        lp = body.get("logprobs")
        if isinstance(lp, bool):
            try:
                lp = (int(body.get("top_logprobs", 0) or 0)) if lp else None
            except (TypeError, ValueError, OverflowError):
                raise ValueError("'top_logprobs' must be an int")
        elif lp is not None:
            try:
                lp = int(lp)
            except (TypeError, ValueError, OverflowError):
                raise ValueError("'logprobs' must be an int or bool")
        if lp is not None and not (0 <= lp <= 20):
            raise ValueError("logprobs must be in [0, 20], got {}".format(lp))
        constraint = None
        if guided:
            # the engine serves guided decoding: response_format json modes
            # and the guided_* / structured_outputs fields become a grammar
            from .guided import constraint_from_request

            constraint = constraint_from_request(body)
        else:
            from .guided import GUIDED_FIELDS

            for key in GUIDED_FIELDS:
                if body.get(key) is not None:
                    raise ValueError(
                        "'{}' needs guided decoding, which this endpoint "
                        "does not enable (set guided_decoding: true in the "
                        "model card or aux config)".format(key))
        rf = body.get("response_format")
        if not guided and rf and isinstance(rf, dict) \
                and rf.get("type") not in (None, "text"):
            # grammar-constrained decoding (json_object/json_schema) is not
            # implemented; refuse instead of silently returning free text
            raise ValueError(
                "response_format '{}' is not supported (no guided-decoding "
                "backend); omit it or use {{'type': 'text'}}".format(
                    rf.get("type")))
        stop = body.get("stop") or []
        if isinstance(stop, str):
            stop = [stop]
        if not isinstance(stop, (list, tuple)) \
                or not all(isinstance(s, str) for s in stop):
            raise ValueError("'stop' must be a string or list of strings")
        stop_ids = body.get("stop_token_ids") or []
        if not isinstance(stop_ids, (list, tuple)):
            raise ValueError("'stop_token_ids' must be a list of ints")
        try:
            stop_ids = [int(t) for t in stop_ids]
        except (TypeError, ValueError, OverflowError):
            raise ValueError("'stop_token_ids' must be a list of ints")
        ignore_eos = bool(body.get("ignore_eos", False))
        if constraint is not None:
            if ignore_eos:
                raise ValueError("guided decoding cannot be combined with "
                                 "ignore_eos (the grammar decides the end)")
            if min_tokens > 0:
                raise ValueError("guided decoding cannot be combined with "
                                 "min_tokens > 0")
        return cls(
            temperature=temperature,
            top_k=top_k,
            top_p=top_p,
            max_tokens=max_tokens,
            stop_token_ids=stop_ids,
            stop=[s for s in stop if s],
            ignore_eos=ignore_eos,
            seed=seed,
            presence_penalty=presence,
            frequency_penalty=frequency,
            repetition_penalty=repetition,
            logprobs=lp,
            min_tokens=min_tokens,
            guided=constraint,
        )


@dataclass
class LlmEngineConfig:
    arch: str = "llama"
    preset: str = "llama-3-8b"
    overrides: Dict[str, Any] = field(default_factory=dict)
    dtype: str = "bfloat16"
    block_size: int = 16
    max_num_seqs: int = 64
    max_model_len: int = 4096
    max_prefill_tokens: int = 8192
    prefill_chunk: int = 2048  # max prefill tokens per step (decode
                               # interleaves between chunks of long prompts)
    gpu_memory_fraction: float = 0.85
    num_kv_blocks: Optional[int] = None  # explicit override (CPU tests)
    quantization: Optional[str] = None   # "fp8": fp8 weights via hipBLASLt
    kv_dtype: str = "bfloat16"  # "fp8": e4m3 KV cache + per-token-per-head
                                # scales -- 2x cached tokens per HBM byte,
                                # half the KV reads on long-context decode
    enable_prefix_caching: bool = False  # vLLM parity: content-addressed
                                # reuse of full prompt KV blocks across
                                # requests sharing a prefix
    weights: Optional[str] = None
    tokenizer_path: Optional[str] = None
    device: Optional[str] = None
    # speculative decoding (vLLM parity): {"method": "ngram",
    # "num_spec_tokens": K, "ngram": N}. Prompt-lookup proposals verified
    # in ONE multi-token forward; EXACT under greedy sampling (accepted
    # tokens equal what step-by-step decode would emit). Off by default;
    # greedy sequences only; TP=1 (sampled/TP requests use plain decode).
    speculative: Optional[Dict[str, Any]] = None
    decode_graphs: bool = True  # capture decode steps into hipGraphs per
                                # batch bucket (GPU, TP=1): collapses the
                                # ~350 Python-dispatched launches of a
                                # llama-8B decode step into one replay
    # multi-LoRA serving (vLLM parity): [{"name": ..., "path": ...}] PEFT
    # adapter directories served on this one base model; a request picks
    # one through the OpenAI "model" field. Relative paths resolve against
    # the model directory. llama family, bf16/fp32 weights, TP=1.
    lora_modules: Optional[List[Dict[str, str]]] = None
    max_lora_rank: int = 16
    # guided decoding (vLLM parity): response_format json_object /
    # json_schema, guided_json / guided_regex / guided_choice and
    # structured_outputs constrain the output to a grammar (guided.py);
    # per-state token bitmasks live in a device bank of guided_mask_slots
    # rows consumed by the token_mask kernels. Off by default. TP=1;
    # byte-level BPE or the built-in byte tokenizer.
    guided_decoding: bool = False
    guided_mask_slots: int = 1024    # >= max_num_seqs
    guided_max_states: int = 20000   # DFA size cap per constraint
    guided_json_depth: int = 4       # container nesting bound of free-form
                                     # JSON (json_object, untyped values)

    @classmethod
    def from_aux(cls, model_path: Optional[str], aux: Dict[str, Any]):
        cfg = cls()
        card: Dict[str, Any] = {}
        if model_path:
            if os.path.isdir(model_path):
                for name in ("model_card.json", "card.json"):
                    p = os.path.join(model_path, name)
                    if os.path.exists(p):
                        with open(p) as f:
                            card = json.load(f)
                        break
                tok = os.path.join(model_path, "tokenizer.json")
                if os.path.exists(tok):
                    cfg.tokenizer_path = tok
                w = os.path.join(model_path, "model.safetensors")
                if os.path.exists(w):
                    cfg.weights = w
            elif model_path.endswith(".json"):
                with open(model_path) as f:
                    card = json.load(f)
        for key in ("arch", "preset", "dtype", "block_size", "max_num_seqs",
                    "max_model_len", "max_prefill_tokens", "prefill_chunk",
                    "gpu_memory_fraction", "num_kv_blocks", "quantization",
                    "kv_dtype", "weights", "device", "decode_graphs",
                    "speculative", "enable_prefix_caching", "lora_modules",
                    "max_lora_rank", "guided_decoding", "guided_mask_slots",
                    "guided_max_states", "guided_json_depth"):
            for src in (card, aux):
                if key in src and src[key] is not None:
                    setattr(cfg, key, src[key])
        cfg.overrides = {**card.get("overrides", {}),
                         **(aux.get("overrides") or {})}
        if cfg.lora_modules:
            base_dir = (model_path if model_path and os.path.isdir(model_path)
                        else os.path.dirname(model_path or ""))
            cfg.lora_modules = [
                {**m, "path": os.path.join(base_dir, str(m.get("path", "")))}
                if isinstance(m, dict) else m  # start() rejects non-dicts
                for m in cfg.lora_modules]
        return cfg


# seq.blocks entry of a page that sliding-window reclamation has returned
# to the allocator: the list keeps its logical indexing, every consumer
# skips the sentinel, and plans carry a valid page id in its place
FREED_BLOCK = -1


class BlockAllocator:
    def __init__(self, num_blocks: int):
        self.num_blocks = num_blocks
        self._free = list(range(num_blocks - 1, -1, -1))

    def alloc(self, n: int) -> List[int]:
        if n > len(self._free):
            raise RuntimeError("KV cache exhausted")
        return [self._free.pop() for _ in range(n)]

    def free(self, blocks: List[int]) -> None:
        self._free.extend(blocks)

    @property
    def available(self) -> int:
        return len(self._free)


class PrefixCacheAllocator(BlockAllocator):
    """Automatic prefix caching (vLLM parity, ``enable_prefix_caching``):
    FULL prompt blocks are content-addressed by the chain hash of their
    token ids, so a request sharing a prompt prefix with an earlier one
    reuses the cached K/V pages and skips their prefill compute.

    Invariants that keep this exact:
    - only FULL blocks are ever shared, and a block's position range is
      determined by its index in the chain, so reuse is always
      position-consistent (RoPE/learned positions bake absolute positions
      into K/V);
    - shared blocks are never written: a sequence's own writes start at
      its first un-cached position (partial final blocks are always
      owned), and decode/speculative writes happen at positions past the
      prompt;
    - at least one prompt token is always left to prefill so the
      first-token logits exist (ncached <= len(prompt) - 1).

    Freed cached blocks keep their contents and move to an LRU of
    evictable blocks; allocation takes never-cached free blocks first and
    evicts LRU entries (dropping their hash) under pressure."""

    def __init__(self, num_blocks: int, block_size: int):
        super().__init__(num_blocks)
        self.block_size = block_size
        self._hash2block: Dict[int, int] = {}
        self._meta: Dict[int, list] = {}   # block -> [chain_hash, refcount]
        self._lru: "OrderedDict[int, None]" = OrderedDict()  # refcount==0
        self.hits = 0        # cached blocks reused
        self.hit_tokens = 0  # prompt tokens skipped

    def _chain_hashes(self, prompt_ids: List[int],
                      salt: int = 0) -> List[int]:
        # ``salt`` seeds the chain: K/V depends on the LoRA adapter, so each
        # adapter hashes into its own block namespace (0 = base model)
        bs = self.block_size
        out = []
        h = salt
        for i in range(len(prompt_ids) // bs):
            h = hash((h, tuple(prompt_ids[i * bs:(i + 1) * bs])))
            out.append(h)
        return out

    def match(self, prompt_ids: List[int], salt: int = 0):
        """Longest cached chain for this prompt -> (block_ids, n_tokens,
        chain_hash at the match point); matched blocks are ref'd
        (protected from eviction) immediately."""
        blocks: List[int] = []
        hashes = self._chain_hashes(prompt_ids, salt)
        for h in hashes:
            b = self._hash2block.get(h)
            if b is None:
                break
            blocks.append(b)
        # never cache-hit the WHOLE prompt: the last token must prefill so
        # its logits exist for first-token sampling
        while blocks and len(blocks) * self.block_size >= len(prompt_ids):
            blocks.pop()
        for b in blocks:
            meta = self._meta[b]
            if meta[1] == 0:
                self._lru.pop(b, None)
            meta[1] += 1
        # hit stats are recorded by the caller on successful admission
        # (a match may be released when the admission budget refuses it)
        chain = hashes[len(blocks) - 1] if blocks else salt
        return blocks, len(blocks) * self.block_size, chain

    def register_block(self, prev_hash: int, tokens: List[int],
                       block_id: int) -> int:
        """Publish ONE full block (prompt or generated) for reuse; returns
        the advanced chain hash. First writer wins: content already
        published elsewhere leaves this copy private."""
        h = hash((prev_hash, tuple(tokens)))
        if h not in self._hash2block and block_id not in self._meta:
            self._hash2block[h] = block_id
            self._meta[block_id] = [h, 1]  # the registering holder's ref
        return h

    def alloc(self, n: int) -> List[int]:
        out: List[int] = []
        for _ in range(n):
            if self._free:
                out.append(self._free.pop())
            elif self._lru:
                b, _ = self._lru.popitem(last=False)  # evict oldest
                h = self._meta.pop(b)[0]
                self._hash2block.pop(h, None)
                out.append(b)
            else:
                self._free.extend(out)
                raise RuntimeError("KV cache exhausted")
        return out

    def free(self, blocks: List[int]) -> None:
        for b in blocks:
            meta = self._meta.get(b)
            if meta is None:
                self._free.append(b)  # never cached: plain free
            else:
                meta[1] -= 1
                if meta[1] <= 0:
                    self._lru[b] = None  # evictable, contents kept

    @property
    def available(self) -> int:
        return len(self._free) + len(self._lru)


class Sequence:
    def __init__(self, req_id: str, prompt_ids: List[int],
                 params: SamplingParams, lora_idx: int = -1,
                 cache_salt: int = 0):
        self.req_id = req_id
        # LoRA adapter slot in the engine's bank (-1 = base model) and the
        # prefix-cache chain seed that goes with it; both survive preemption
        self.lora_idx = lora_idx
        self.cache_salt = cache_salt
        self.prompt_ids = prompt_ids
        self.output_ids: List[int] = []
        self.generated = 0  # survives preemption (output folds into prompt)
        self.prefilled = 0  # prompt tokens already in the KV cache
        self.params = params
        self.blocks: List[int] = []
        # sliding window: blocks[:swa_freed] are FREED_BLOCK sentinels
        self.swa_freed = 0
        self.stream: "asyncio.Queue" = asyncio.Queue()
        self.finished = False
        self.finish_reason: Optional[str] = None
        self.created = time.time()
        self.first_token_time: Optional[float] = None
        self.spec_misses = 0  # consecutive fully-rejected proposals
        # prefix-cache registration progress: tokens covered by published
        # blocks, and the chain hash at that point
        self.cached_upto = 0
        self.cache_hash = 0
        self.text_sent = 0  # chars of decoded output already streamed
        # guided decoding: guided.GuidedState (grammar + DFA state). Lives
        # on the sequence, so it survives preemption and recompute
        self.guided = None

    def __len__(self):
        return len(self.prompt_ids) + len(self.output_ids)


class LlmEngine:
    def __init__(self, cfg: LlmEngineConfig):
        self.cfg = cfg
        if cfg.device:
            self.device = torch.device(cfg.device)
        elif torch.cuda.is_available():
            from ..torch_engine import _pick_device

            # most-free-HBM placement (multi-model nodes spread engines)
            self.device = _pick_device({})
        else:
            self.device = torch.device("cpu")
        self.dtype = (torch.bfloat16 if self.device.type == "cuda"
                      else torch.float32)
        self.model: Optional[LlamaForCausalLM] = None
        self.kv_caches: List = []
        self.allocator: Optional[BlockAllocator] = None
        self.tokenizer = None
        self.waiting: List[Sequence] = []
        self.running: List[Sequence] = []
        # aborts cross threads (event loop -> step worker): appended on the
        # loop, drained at the top of step() -- deque ops are GIL-atomic
        self._aborted: "deque[Sequence]" = deque()
        # serializes GPU execution between the step worker thread and the
        # non-generative paths (embed/pooling): both launch on the default
        # stream, and a forward issued from a second thread while a decode
        # hipGraph is being captured corrupts the capture; under TP it
        # would also interleave two plan broadcasts (rank-order corruption)
        self._exec_lock = threading.Lock()
        self._loop_task: Optional[asyncio.Task] = None
        self._wake: Optional[asyncio.Event] = None
        self._started = False
        self._stopped = False
        # decode hipGraphs: one per batch bucket, shared memory pool
        self._decode_graphs: Dict[int, Dict[str, Any]] = {}
        self._decode_pin: Dict[int, Dict[str, Any]] = {}
        self._graph_pool = None
        self._decode_buckets = [n for n in
                                (1, 2, 4, 8, 16, 24, 32, 48, 64, 96, 128,
                                 192, 256)
                                if n < self.cfg.max_num_seqs]
        self._decode_buckets.append(self.cfg.max_num_seqs)
        self.stats = {"prompt_tokens": 0, "generated_tokens": 0, "steps": 0,
                      "prefill_batches": 0, "decode_batches": 0,
                      "preemptions": 0, "aborts": 0,
                      "graph_captures": 0, "graph_replays": 0,
                      "spec_proposed": 0, "spec_accepted": 0,
                      "lora_requests": 0, "swa_blocks_freed": 0}
        # multi-LoRA: models.lora.LoraBank built by start() when
        # cfg.lora_modules is set; None = every path below runs as before
        self.lora_bank = None
        # sliding-window width of the served model (LlamaConfig), set by
        # start(); 0 = full context, no KV page reclamation
        self._window = 0
        # guided decoding: guided.GuidedCompiler + guided.MaskBank built by
        # start() when cfg.guided_decoding is set; None = off
        self.guided_compiler = None
        self.mask_bank = None
        self._dead_end_logged = False

    # ------------------------------------------------------------------ #
    def start(self) -> None:
        if self._started:
            return
        cfg = self.cfg
        # TP over RCCL/xGMI: one process per GPU (torchrun); every rank
        # builds its shard, rank 0 owns scheduling + the HTTP front
        from ...parallel import tp as tp_mod

        self.tp_size = tp_mod.world_size()
        self.tp_rank = tp_mod.rank()
        torch.manual_seed(1234)  # identical replicated params across ranks
        gpt2 = (str(cfg.arch).lower() == "gpt2"
                or str(cfg.preset).startswith("gpt2"))
        self._check_sliding_window(gpt2)
        if not gpt2:
            self._check_moe_options()
        lora_adapters = (self._load_lora_adapters(gpt2)
                         if cfg.lora_modules else None)
        if gpt2:
            # GPT-2 family: same engine-facing forward interface as llama
            # (paged kv_caches + attn_ctx modes), so scheduling, chunked
            # prefill, decode graphs and speculation serve it unchanged
            from ...models.gpt2 import PRESETS as GPT2_PRESETS
            from ...models.gpt2 import GPT2Config, GPT2ForCausalLM

            if self.tp_size > 1:
                raise ValueError(
                    "tensor parallelism is implemented for the llama "
                    "family only (arch=gpt2 serves at tp=1)")
            mcfg = GPT2Config(**{**GPT2_PRESETS[cfg.preset].__dict__,
                                 **cfg.overrides})
            self.model_config = mcfg
            if cfg.max_model_len > mcfg.max_position:
                # learned absolute positions END at max_position: serving
                # beyond it would silently clamp position ids
                print("[llm] gpt2 max_model_len capped to max_position "
                      "({} -> {})".format(cfg.max_model_len,
                                          mcfg.max_position))
                cfg.max_model_len = mcfg.max_position
            model = GPT2ForCausalLM(mcfg)
        else:
            mcfg = LlamaConfig(**{**PRESETS[cfg.preset].__dict__,
                                  **cfg.overrides})
            self.model_config = mcfg
            self._window = int(mcfg.sliding_window)
            model = LlamaForCausalLM(mcfg, tp_rank=self.tp_rank,
                                     tp_size=self.tp_size)
        if cfg.weights:
            if self.tp_size > 1:
                # full checkpoint -> this rank's shard
                from safetensors.torch import load_file

                full = (load_file(cfg.weights)
                        if cfg.weights.endswith(".safetensors")
                        else torch.load(cfg.weights, map_location="cpu",
                                        weights_only=True))
                from ...models.convert import convert_hf_auto

                model.load_state_dict(tp_mod.shard_llama_weights(
                    convert_hf_auto(full), mcfg, self.tp_rank,
                    self.tp_size))
            else:
                from ...models import load_weights

                load_weights(model, cfg.weights)
        self.model = model.eval().to(self.device).to(self.dtype)
        if cfg.quantization == "fp8":
            if self.device.type != "cuda":
                raise ValueError("fp8 quantization needs a GPU (hipBLASLt)")
            from ...models.quant import quantize_llama_fp8

            n = quantize_llama_fp8(self.model)
            if n == 0:
                raise ValueError(
                    "fp8 quantization covers the llama-family projections "
                    "only (arch '{}' has none)".format(cfg.arch))
            print("[llm] fp8-quantized {} projection layers".format(n))
        if lora_adapters:
            from ...models.lora import LoraBank

            self.lora_bank = LoraBank(lora_adapters, mcfg, cfg.max_lora_rank,
                                      self.device, self.dtype)
            print("[llm] serving {} LoRA adapters: {}".format(
                len(self.lora_bank), ", ".join(self.lora_bank.names)))

        self.tokenizer = (HfTokenizer(cfg.tokenizer_path)
                          if cfg.tokenizer_path else SimpleTokenizer())
        if cfg.guided_decoding:
            self._start_guided(mcfg)

        # KV cache sizing from free HBM (heads sharded under TP)
        bs = cfg.block_size
        kv_heads = mcfg.kv_heads // self.tp_size
        fp8_kv = str(cfg.kv_dtype).lower() in ("fp8", "float8", "e4m3")
        kv_itemsize = 1 if fp8_kv else self.dtype.itemsize
        per_block_bytes = (2 * kv_heads * bs *
                           (mcfg.head_dim * kv_itemsize +
                            (4 if fp8_kv else 0)) * mcfg.layers)
        if cfg.num_kv_blocks:
            num_blocks = int(cfg.num_kv_blocks)
        elif self.device.type == "cuda":
            free, _ = torch.cuda.mem_get_info(self.device)
            budget = int(free * cfg.gpu_memory_fraction)
            num_blocks = max(budget // per_block_bytes, 64)
        else:
            num_blocks = 512
        if self.tp_size > 1:
            # all ranks must agree on capacity: take the global minimum
            import torch.distributed as dist

            t = torch.tensor([num_blocks], dtype=torch.long,
                             device=self.device if self.device.type == "cuda"
                             else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            num_blocks = int(t.item())
        self.allocator = (PrefixCacheAllocator(num_blocks, bs)
                          if cfg.enable_prefix_caching
                          else BlockAllocator(num_blocks))
        if fp8_kv:
            # 4-tuple per layer: e4m3 byte caches + f32 [NB, Hkv, BS]
            # per-token-per-head scales (written by kv_cache_write's
            # wave-per-head absmax quantizer, attention_decode.hip)
            self.kv_caches = [
                (torch.zeros(num_blocks, kv_heads, bs, mcfg.head_dim,
                             dtype=torch.uint8, device=self.device),
                 torch.zeros(num_blocks, kv_heads, bs, mcfg.head_dim,
                             dtype=torch.uint8, device=self.device),
                 torch.ones(num_blocks, kv_heads, bs,
                            dtype=torch.float32, device=self.device),
                 torch.ones(num_blocks, kv_heads, bs,
                            dtype=torch.float32, device=self.device))
                for _ in range(mcfg.layers)
            ]
        else:
            self.kv_caches = [
                (torch.zeros(num_blocks, kv_heads, bs, mcfg.head_dim,
                             dtype=self.dtype, device=self.device),
                 torch.zeros(num_blocks, kv_heads, bs, mcfg.head_dim,
                             dtype=self.dtype, device=self.device))
                for _ in range(mcfg.layers)
            ]
        if self.tp_size > 1:
            from .plan_codec import PlanCodec

            self._plan_codec = PlanCodec(cfg, self.device)
        self._started = True

    def _check_sliding_window(self, gpt2: bool) -> None:
        """Validate a ``sliding_window`` override before anything is built.
        Model cards carry the key with null for full context (released
        Mixtral cards do): null is dropped so the preset's value stands."""
        cfg = self.cfg
        if "sliding_window" not in cfg.overrides:
            return
        window = cfg.overrides["sliding_window"]
        if window is None:
            cfg.overrides = {k: v for k, v in cfg.overrides.items()
                             if k != "sliding_window"}
            return
        if gpt2:
            raise ValueError(
                "sliding_window={} is not supported for arch=gpt2: the "
                "window is implemented for the llama family".format(window))
        if isinstance(window, bool) or not isinstance(window, int) \
                or window < 0:
            raise ValueError(
                "sliding_window must be a non-negative integer or null, "
                "got {!r}".format(window))

    def _check_moe_options(self) -> None:
        """Refuse, before anything is built or read, what the MoE path does
        not implement (cfg.overrides may declare an MoE of any size)."""
        cfg = self.cfg
        base = PRESETS.get(cfg.preset)
        n_exp = int(cfg.overrides.get(
            "num_experts", base.num_experts if base is not None else 0))
        if n_exp <= 0:
            return
        window = cfg.overrides.get(
            "sliding_window", base.sliding_window if base is not None else 0)
        if window:
            # dense cards only: the windowed path is not validated against
            # a Mixtral reference, and released Mixtral cards set null
            raise ValueError(
                "sliding_window={} is not supported for mixture-of-experts "
                "models (num_experts={})".format(window, n_exp))
        if cfg.quantization == "fp8":
            raise ValueError(
                "quantization='fp8' is not supported for mixture-of-experts "
                "models (num_experts={}): the expert kernels are bf16".format(
                    n_exp))
        if cfg.lora_modules:
            raise ValueError(
                "lora_modules are not supported for mixture-of-experts "
                "models (num_experts={})".format(n_exp))
        if self.tp_size > 1:
            raise ValueError(
                "tensor parallelism (tp_size={}) is not supported for "
                "mixture-of-experts models (num_experts={}): experts are "
                "not sharded".format(self.tp_size, n_exp))

    # ------------------------------------------------------------------ #
    # guided decoding (guided.py; kernels ops/csrc/token_mask.hip)
    # ------------------------------------------------------------------ #
    def _start_guided(self, mcfg) -> None:
        from .guided import GuidedCompiler, MaskBank

        cfg = self.cfg
        if self.tp_size > 1:
            raise ValueError("guided_decoding is not supported under tensor "
                             "parallelism (tp_size={})".format(self.tp_size))
        if int(cfg.guided_mask_slots) < int(cfg.max_num_seqs):
            raise ValueError(
                "guided_mask_slots ({}) must be >= max_num_seqs ({}): one "
                "step can need a mask per running sequence".format(
                    cfg.guided_mask_slots, cfg.max_num_seqs))
        # raises ValueError for tokenizers whose tokens are not bytes
        self.guided_compiler = GuidedCompiler(
            self.tokenizer, int(mcfg.vocab_size),
            max_states=int(cfg.guided_max_states),
            json_depth=int(cfg.guided_json_depth))
        for key in ("guided_requests", "guided_mask_hits",
                    "guided_mask_misses", "guided_dead_ends"):
            self.stats[key] = 0
        self.mask_bank = MaskBank(int(cfg.guided_mask_slots),
                                  self.guided_compiler.vocab.words,
                                  self.device, self.stats)

    def _guided_state(self, params: SamplingParams):
        """GuidedState for a request's constraint (compile is LRU-cached)."""
        from .guided import GuidedState

        if self.guided_compiler is None:
            raise ValueError(
                "this endpoint does not enable guided decoding (set "
                "guided_decoding: true in the model card or aux config)")
        if params.ignore_eos or params.min_tokens > 0:
            raise ValueError("guided decoding cannot be combined with "
                             "ignore_eos or min_tokens > 0")
        grammar = self.guided_compiler.compile(*params.guided)
        return GuidedState(grammar, [self.tokenizer.eos_id]
                           + list(params.stop_token_ids))

    def _note_dead_end(self, s: "Sequence") -> None:
        self.stats["guided_dead_ends"] += 1
        if not self._dead_end_logged:
            self._dead_end_logged = True
            print("[llm] guided decoding dead end: no token of the "
                  "vocabulary continues grammar '{}' (further ones are "
                  "only counted in stats)".format(s.guided.grammar.key[:80]))

    def _finish_dead_end(self, s: "Sequence") -> None:
        """A live grammar state whose mask allows no token (the vocabulary
        cannot spell a required byte): finish instead of sampling."""
        self._note_dead_end(s)
        if not s.finished:
            s.finished = True
            s.finish_reason = "stop"
            s.stream.put_nowait({"token_ids": [], "text": "",
                                 "finished": True, "finish_reason": "stop"})

    # ------------------------------------------------------------------ #
    # multi-LoRA (models/lora.py; kernels ops/csrc/lora.hip)
    # ------------------------------------------------------------------ #
    def _load_lora_adapters(self, gpt2: bool) -> List:
        """Validate cfg.lora_modules and read the adapters (cheap: before
        the base model is built). Combinations this engine does not serve
        raise instead of silently ignoring the adapters."""
        from ...models.lora import load_adapter

        cfg = self.cfg
        if gpt2:
            raise ValueError("lora_modules serve the llama family only "
                             "(arch=gpt2 has no adapter hook)")
        if cfg.quantization == "fp8":
            raise ValueError(
                "lora_modules are not supported with quantization='fp8': "
                "the fp8 path never materialises the bf16 activation the "
                "adapter reads")
        if self.tp_size > 1:
            raise ValueError("lora_modules are not supported under tensor "
                             "parallelism (tp_size={})".format(self.tp_size))
        adapters = []
        for m in cfg.lora_modules:
            if not isinstance(m, dict) or not m.get("name") \
                    or not m.get("path"):
                raise ValueError(
                    "lora_modules entries must be {{'name': ..., 'path': "
                    "...}}, got {!r}".format(m))
            adapters.append(load_adapter(str(m["path"]),
                                         int(cfg.max_lora_rank),
                                         name=str(m["name"])))
        return adapters

    def _resolve_lora(self, model: Any) -> int:
        """OpenAI ``model`` field -> adapter slot; anything that is not a
        configured adapter name serves the base model (-1)."""
        if self.lora_bank is None or not isinstance(model, str):
            return -1
        return self.lora_bank.index.get(model, -1)

    def _lora_ctx(self, attn_ctx: Dict[str, Any], rows: List[int],
                  lens: Optional[List[int]] = None,
                  smax: int = 1) -> None:
        """Expand per-sequence adapter slots to the per-token int32 idx the
        kernels take and attach it to attn_ctx; padded tokens get -1."""
        if lens is None:
            idx = torch.tensor(rows, dtype=torch.int32)
        else:
            idx = torch.full((len(rows), smax), -1, dtype=torch.int32)
            for i, n in enumerate(lens):
                idx[i, :n] = rows[i]
            idx = idx.view(-1)
        attn_ctx["lora"] = (self.lora_bank, idx.to(self.device))

    # ------------------------------------------------------------------ #
    # request API
    # ------------------------------------------------------------------ #
    async def add_request(self, prompt_ids: List[int],
                          params: SamplingParams,
                          lora_idx: int = -1) -> Sequence:
        if self._stopped:
            raise RuntimeError("LLM engine stopped (endpoint was removed)")
        if len(prompt_ids) >= self.cfg.max_model_len:
            raise ValueError(
                "prompt length {} exceeds max_model_len {}".format(
                    len(prompt_ids), self.cfg.max_model_len))
        if params.has_penalties() and getattr(self, "tp_size", 1) > 1:
            # worker ranks hold vocab shards but not the token history the
            # penalties need; fail loudly instead of silently ignoring
            raise ValueError(
                "presence/frequency/repetition penalties are not supported "
                "under tensor parallelism yet")
        if params.logprobs is not None and getattr(self, "tp_size", 1) > 1:
            raise ValueError(
                "logprobs need a full-vocab softmax and are not supported "
                "under tensor parallelism yet")
        if params.min_tokens > 0 and getattr(self, "tp_size", 1) > 1:
            raise ValueError(
                "min_tokens is not supported under tensor parallelism yet")
        guided_state = (self._guided_state(params)
                        if params.guided is not None else None)
        if lora_idx >= 0:
            if self.lora_bank is None or lora_idx >= len(self.lora_bank):
                raise ValueError("no LoRA adapter in slot {}".format(lora_idx))
            seq = Sequence(uuid.uuid4().hex, prompt_ids, params,
                           lora_idx=lora_idx,
                           cache_salt=self.lora_bank.salts[lora_idx])
            self.stats["lora_requests"] += 1
        else:
            seq = Sequence(uuid.uuid4().hex, prompt_ids, params)
        if guided_state is not None:
            seq.guided = guided_state
            self.stats["guided_requests"] += 1
        self.waiting.append(seq)
        self._ensure_loop()
        self._wake.set()
        return seq

    def abort(self, seq: "Sequence") -> None:
        """Stop generating for a sequence (client gone).

        Runs on the event loop while step() runs in a worker thread
        (asyncio.to_thread), so scheduler state is NOT mutated here: the
        sequence goes onto a thread-safe queue that step() drains at its
        top, keeping all waiting/running/allocator mutation on the step
        thread (a mid-_admit list removal here could make _admit pop and
        drop a different queued sequence, hanging its client forever)."""
        seq.finished = True
        seq.finish_reason = seq.finish_reason or "abort"
        self._aborted.append(seq)
        self.stats["aborts"] = self.stats.get("aborts", 0) + 1
        if self._wake is not None:
            self._wake.set()  # free the pages promptly even when idle

    async def generate(self, prompt: str, params: SamplingParams,
                       lora_idx: int = -1
                       ) -> AsyncGenerator[Dict[str, Any], None]:
        ids = self.tokenizer.encode(prompt)
        seq = await self.add_request(ids, params, lora_idx)
        try:
            while True:
                item = await seq.stream.get()
                yield item
                if item.get("finished"):
                    return
        finally:
            # consumer cancelled/disconnected mid-stream: stop generating
            if not seq.finished:
                self.abort(seq)

    async def generate_simple(self, body: Dict[str, Any]) -> Dict[str, Any]:
        """Non-OpenAI route: {"prompt": str, "max_tokens": ...}; an
        optional "lora" key names a configured adapter."""
        prompt = body.get("prompt") or body.get("text") or ""
        params = SamplingParams.from_request(
            body, guided=self.cfg.guided_decoding)
        tokens: List[int] = []
        reason = None
        async for item in self.generate(prompt, params,
                                        self._resolve_lora(body.get("lora"))):
            if item.get("error"):
                raise RuntimeError("generation failed: {}".format(
                    item["error"]))
            tokens.extend(item.get("token_ids", []))
            reason = item.get("finish_reason") or reason
        return {
            "text": self._truncate_at_stop(
                self.tokenizer.decode(tokens), params, reason),
            "tokens": len(tokens),
        }

    # ------------------------------------------------------------------ #
    # engine loop
    # ------------------------------------------------------------------ #
    def _ensure_loop(self) -> None:
        loop = asyncio.get_running_loop()
        if (self._loop_task is None
                or getattr(self, "_loop_ref", None) is not loop
                or self._loop_task.done()):  # restart after a step crash
            self._loop_ref = loop
            self._wake = asyncio.Event()
            self._loop_task = loop.create_task(self._engine_loop())

    def stop(self) -> None:
        """Thread-safe teardown (endpoint removed on a config reload):
        cancel the scheduler loop, poison active sequences so no client
        hangs, and drop the model + KV cache references so their HBM frees
        with the processor's post-flush gc."""
        self._stopped = True
        task, loop = self._loop_task, getattr(self, "_loop_ref", None)
        self._loop_task = None
        waiting, running = self.waiting, self.running
        self.waiting, self.running = [], []

        def _teardown():
            if task is not None and not task.done():
                task.cancel()
            for seq in waiting + running:
                seq.stream.put_nowait({"error": "engine stopped",
                                       "finished": True, "token_ids": []})

        if loop is not None and not loop.is_closed():
            loop.call_soon_threadsafe(_teardown)
        self.tp_shutdown()
        self._decode_graphs.clear()
        self._decode_pin.clear()
        self._graph_pool = None
        self.kv_caches = []
        self.model = None

    async def _engine_loop(self) -> None:
        while True:
            if not self.waiting and not self.running:
                self._wake.clear()
                await self._wake.wait()
            try:
                await asyncio.to_thread(self.step)
            except Exception as ex:
                # poison every active sequence rather than hanging clients;
                # return their KV pages before dropping them
                for seq in self.waiting + self.running:
                    seq.stream.put_nowait(
                        {"error": str(ex), "finished": True, "token_ids": []})
                    self._free_blocks(seq)
                self.waiting.clear()
                self.running.clear()
                raise
            # hand emitted tokens to the event loop promptly
            await asyncio.sleep(0)

    # ------------------------------------------------------------------ #
    def step(self) -> None:
        """One scheduler iteration: admit, prefill (chunked -- at most
        ``prefill_chunk`` prompt tokens per step so decode latency stays
        bounded under long-prompt load), then decode everything else."""
        with self._exec_lock:
            self._step_locked()

    def _step_locked(self) -> None:
        self.stats["steps"] += 1
        self._drain_aborts()
        self._admit()
        budget = self.cfg.prefill_chunk
        pending = [s for s in self.running
                   if s.prefilled < len(s.prompt_ids)]
        # fresh short prompts batch through the dense prefill path
        fresh = []
        for s in pending:
            need = len(s.prompt_ids)
            if s.prefilled == 0 and need <= budget:
                fresh.append(s)
                budget -= need
        if fresh:
            self._prefill(fresh)
            for s in fresh:
                s.prefilled = len(s.prompt_ids)
                self._register_prefix(s)
        # long/continuing prompts advance by chunks (batched paged
        # attention against their cached histories)
        cont = [s for s in pending if s not in fresh]
        if cont and budget > 0:
            self._prefill_chunk(cont, budget)
        decoding = [s for s in self.running if not s.finished
                    and s.prefilled >= len(s.prompt_ids) and s.output_ids]
        if decoding:
            spec_k = self._spec_tokens()
            if spec_k and getattr(self, "tp_size", 1) <= 1:
                # speculative path: greedy sequences only (acceptance is
                # exact for argmax); sampled or penalized sequences take
                # plain decode (penalties change the argmax per position)
                spec = [s for s in decoding if s.params.temperature == 0.0
                        and not s.params.has_penalties()
                        and s.params.logprobs is None
                        and s.params.min_tokens <= s.generated
                        and s.guided is None]
                rest = [s for s in decoding if s not in spec]
            else:
                spec, rest = [], decoding
            if spec:
                self._decode_spec(spec, spec_k)
            if rest:
                self._decode(rest)
        for s in list(self.running):
            self._register_prefix(s)  # publish newly-FILLED blocks
            if s.finished:
                self.running.remove(s)
                self._free_blocks(s)
            else:
                # after _register_prefix, so a page is published (and stays
                # matchable) before it goes back through allocator.free
                self._reclaim_window(s)

    def _free_blocks(self, seq: Sequence) -> None:
        """Return every page the sequence still holds (window-reclaimed
        entries were freed when they became sentinels)."""
        held = [b for b in seq.blocks if b != FREED_BLOCK]
        if held:
            self.allocator.free(held)
        seq.blocks = []
        seq.swa_freed = 0

    def _reclaim_window(self, s: Sequence) -> None:
        """Sliding window: free the pages no future query of ``s`` can see.
        The next query sits at position p (the next chunk's first position
        mid-prefill, else the newest token, whose K/V is written on its
        step); it and every later query see only keys > p - window, so
        page j is dead once (j + 1) * block_size <= p - window + 1."""
        if not self._window or not s.blocks:
            return
        if s.prefilled < len(s.prompt_ids):
            p = s.prefilled
        else:
            p = len(s) - 1
        dead = min((p - self._window + 1) // self.cfg.block_size,
                   len(s.blocks))
        if dead <= s.swa_freed:
            return
        self.allocator.free(s.blocks[s.swa_freed:dead])
        s.blocks[s.swa_freed:dead] = [FREED_BLOCK] * (dead - s.swa_freed)
        self.stats["swa_blocks_freed"] += dead - s.swa_freed
        s.swa_freed = dead

    @staticmethod
    def _block_table(s: Sequence) -> List[int]:
        """Block-table row for a plan (TP codec, device tables, decode-graph
        statics): window-reclaimed entries, which the kernels never read,
        carry page 0 so the table holds only in-range ids."""
        return [0 if b == FREED_BLOCK else b for b in s.blocks]

    def _drain_aborts(self) -> None:
        """Apply aborts queued by abort() -- all scheduler-state mutation
        happens here on the step thread."""
        while True:
            try:
                seq = self._aborted.popleft()
            except IndexError:
                return
            if seq in self.waiting:
                self.waiting.remove(seq)
            if seq in self.running:
                self.running.remove(seq)
            self._free_blocks(seq)

    def _admit(self) -> List[Sequence]:
        admitted: List[Sequence] = []
        tokens = 0
        bs = self.cfg.block_size
        prefix_cache = isinstance(self.allocator, PrefixCacheAllocator)
        while self.waiting and len(self.running) < self.cfg.max_num_seqs:
            seq = self.waiting[0]
            if seq.finished:  # aborted after the drain at step() top
                self.waiting.pop(0)
                continue
            cached: List[int] = []
            ncached = 0
            chain = 0
            if prefix_cache:
                cached, ncached, chain = self.allocator.match(
                    seq.prompt_ids, seq.cache_salt)
            need = len(seq.prompt_ids) - ncached
            if admitted and tokens + need > self.cfg.max_prefill_tokens:
                if cached:
                    self.allocator.free(cached)  # un-ref the match
                break
            total_blocks = (len(seq.prompt_ids) + bs - 1) // bs
            need_blocks = total_blocks - len(cached)
            # keep one spare block per running seq for decode growth
            if need_blocks + len(self.running) + 1 > self.allocator.available:
                if cached:
                    self.allocator.free(cached)
                break
            seq.blocks = cached + self.allocator.alloc(need_blocks)
            seq.swa_freed = 0
            seq.prefilled = ncached  # cached prefix skips its prefill
            # registration chain restarts at the match point (also resets
            # stale state on preemption re-admission)
            seq.cached_upto = ncached
            seq.cache_hash = chain
            if prefix_cache and ncached:
                self.allocator.hits += len(cached)
                self.allocator.hit_tokens += ncached
                self.stats["prefix_cache_hit_tokens"] = (
                    self.stats.get("prefix_cache_hit_tokens", 0) + ncached)
            self.waiting.pop(0)
            self.running.append(seq)
            admitted.append(seq)
            tokens += need
        return admitted

    def _register_prefix(self, s: Sequence) -> None:
        """Publish every full block whose K/V is in the cache -- prompt
        AND generated tokens (multi-turn chat resends assistant output as
        the next prompt, so generated blocks are reusable prefixes too).
        KV availability: mid-prefill only the first ``prefilled`` tokens
        are written; once the prompt is done, everything except the
        newest token (written on its NEXT step) is."""
        alloc = self.allocator
        if not isinstance(alloc, PrefixCacheAllocator):
            return
        bs = alloc.block_size
        if s.prefilled < len(s.prompt_ids):
            avail = s.prefilled
        else:
            avail = len(s.prompt_ids) + max(len(s.output_ids) - 1, 0)
        if s.cached_upto + bs > avail:
            return
        toks = s.prompt_ids + s.output_ids
        while s.cached_upto + bs <= avail:
            blk = s.cached_upto // bs
            tokens = toks[s.cached_upto:s.cached_upto + bs]
            if s.blocks[blk] == FREED_BLOCK:
                # window-reclaimed before it was published (cannot happen in
                # step order; kept safe): only the chain hash advances
                s.cache_hash = hash((s.cache_hash, tuple(tokens)))
            else:
                s.cache_hash = alloc.register_block(
                    s.cache_hash, tokens, s.blocks[blk])
            s.cached_upto += bs

    def _slot(self, seq: Sequence, pos: int) -> int:
        bs = self.cfg.block_size
        blk = seq.blocks[pos // bs]
        if blk == FREED_BLOCK:
            raise RuntimeError(
                "position {} lies in a page the sliding window already "
                "reclaimed".format(pos))
        return blk * bs + pos % bs

    def _sample_spec(self, seqs: List[Sequence]) -> List[tuple]:
        step_seed = random.getrandbits(31)
        # a request-level seed makes the sequence reproducible: vary it per
        # emitted token (seed + generated) so steps draw fresh noise
        return [(s.params.temperature, s.params.top_k, s.params.top_p,
                 (s.params.seed + s.generated) & 0x7FFFFFFF
                 if s.params.seed is not None else step_seed)
                for s in seqs]

    def _prefill(self, seqs: List[Sequence]) -> None:
        self.stats["prefill_batches"] += 1
        plan = {
            "mode": "prefill",
            "prompts": [list(s.prompt_ids) for s in seqs],
            "slots": [[self._slot(s, p) for p in range(len(s.prompt_ids))]
                      for s in seqs],
            "sample": self._sample_spec(seqs),
        }
        if self.lora_bank is not None:
            plan["lora"] = [s.lora_idx for s in seqs]
        self._tp_broadcast(plan)
        logits = self._exec_prefill(plan)
        self.stats["prompt_tokens"] += sum(len(p) for p in plan["prompts"])
        self._sample_and_emit(seqs, logits, sample=plan["sample"])

    def _prefill_chunk(self, seqs: List["Sequence"], budget: int) -> None:
        """Advance several sequences' prefill by up to ``budget`` tokens
        total in ONE batched paged-attention forward; samples first tokens
        for the sequences whose chunk completes the prompt.

        Fair-share: the budget splits evenly across chunking prompts (then
        leftovers go FCFS), so a newly arrived long prompt advances every
        step instead of starving behind an earlier prompt's remaining
        chunks (round-1 packed strictly FCFS)."""
        batch = []
        if len(seqs) > 1:
            share = max(budget // len(seqs), 1)
            remaining = budget
            needs = []
            for s in seqs:
                if remaining <= 0:
                    break
                need = len(s.prompt_ids) - s.prefilled
                take = min(share, need, remaining)
                batch.append((s, take))
                needs.append(need - take)
                remaining -= take
            # leftovers (some prompts needed < share) go FCFS
            for i, (s, take) in enumerate(batch):
                if remaining <= 0:
                    break
                extra = min(needs[i], remaining)
                if extra:
                    batch[i] = (s, take + extra)
                    remaining -= extra
        else:
            for s in seqs:
                if budget <= 0:
                    break
                chunk = min(budget, len(s.prompt_ids) - s.prefilled)
                batch.append((s, chunk))
                budget -= chunk
        if not batch:
            return
        self.stats["prefill_batches"] += 1
        plan = {
            "mode": "chunk",
            "tokens": [s.prompt_ids[s.prefilled:s.prefilled + c]
                       for s, c in batch],
            "starts": [s.prefilled for s, c in batch],
            "kv_lens": [s.prefilled + c for s, c in batch],
            "slots": [[self._slot(s, p)
                       for p in range(s.prefilled, s.prefilled + c)]
                      for s, c in batch],
            "blocks": [self._block_table(s) for s, c in batch],
            "complete": [s.prefilled + c >= len(s.prompt_ids)
                         for s, c in batch],
        }
        # sampling spec only for rows whose chunk completes the prompt
        done_seqs = [s for (s, c), comp in zip(batch, plan["complete"])
                     if comp]
        plan["sample"] = self._sample_spec(done_seqs)
        if self.lora_bank is not None:
            plan["lora"] = [s.lora_idx for s, c in batch]
        self._tp_broadcast(plan)
        logits = self._exec_chunk(plan)
        done = []
        for (s, c), complete in zip(batch, plan["complete"]):
            s.prefilled += c
            self.stats["prompt_tokens"] += c
            if complete:
                done.append(s)
                self._register_prefix(s)
        if done:
            self._sample_and_emit(done, logits, sample=plan["sample"])

    @torch.inference_mode()
    def _exec_chunk(self, plan: Dict[str, Any]) -> torch.Tensor:
        dev = self.device
        b = len(plan["tokens"])
        lens = [len(t) for t in plan["tokens"]]
        smax = max(lens)
        tokens = torch.zeros(b, smax, dtype=torch.long)
        positions = torch.zeros(b, smax, dtype=torch.int32)
        slot_map = torch.full((b, smax), -1, dtype=torch.int32)
        for i in range(b):
            n = lens[i]
            tokens[i, :n] = torch.tensor(plan["tokens"][i], dtype=torch.long)
            positions[i, :n] = torch.arange(
                plan["starts"][i], plan["starts"][i] + n, dtype=torch.int32)
            slot_map[i, :n] = torch.tensor(plan["slots"][i],
                                           dtype=torch.int32)
        max_blocks = max(len(bl) for bl in plan["blocks"])
        btab = torch.zeros(b, max_blocks, dtype=torch.int32)
        for i, bl in enumerate(plan["blocks"]):
            btab[i, :len(bl)] = torch.tensor(bl, dtype=torch.int32)
        attn_ctx = {
            "mode": "prefill_paged", "batch": b, "seq": smax,
            "kv_lens": torch.tensor(plan["kv_lens"], dtype=torch.int32,
                                    device=dev),
            "q_lens": torch.tensor(lens, dtype=torch.int32, device=dev),
            "block_table": btab.to(dev),
            "slot_mapping": slot_map.view(-1).to(dev),
        }
        if "lora" in plan:
            self._lora_ctx(attn_ctx, plan["lora"], lens, smax)
        rows = [i * smax + lens[i] - 1
                for i in range(b) if plan["complete"][i]]
        last_idx = torch.tensor(rows, dtype=torch.long, device=dev)
        return self.model(tokens.view(-1).to(dev),
                          positions.view(-1).to(dev),
                          kv_caches=self.kv_caches, attn_ctx=attn_ctx,
                          last_token_idx=last_idx, gather_logits=False)

    @torch.inference_mode()
    def _exec_prefill(self, plan: Dict[str, Any]) -> torch.Tensor:
        prompts = plan["prompts"]
        slots = plan["slots"]
        b = len(prompts)
        lens = [len(p) for p in prompts]
        smax = max(lens)
        dev = self.device

        tokens = torch.zeros(b, smax, dtype=torch.long)
        positions = torch.zeros(b, smax, dtype=torch.int32)
        slot_map = torch.full((b, smax), -1, dtype=torch.int32)
        for i in range(b):
            n = lens[i]
            tokens[i, :n] = torch.tensor(prompts[i], dtype=torch.long)
            positions[i, :n] = torch.arange(n, dtype=torch.int32)
            slot_map[i, :n] = torch.tensor(slots[i], dtype=torch.int32)
        seq_lens = torch.tensor(lens, dtype=torch.int32, device=dev)
        attn_ctx = {
            "mode": "prefill", "batch": b, "seq": smax,
            "seq_lens": seq_lens,
            "slot_mapping": slot_map.view(-1).to(dev),
        }
        if "lora" in plan:
            self._lora_ctx(attn_ctx, plan["lora"], lens, smax)
        last_idx = torch.tensor(
            [i * smax + lens[i] - 1 for i in range(b)], dtype=torch.long,
            device=dev)
        return self.model(
            tokens.view(-1).to(dev), positions.view(-1).to(dev),
            kv_caches=self.kv_caches, attn_ctx=attn_ctx,
            last_token_idx=last_idx, gather_logits=False)

    @torch.inference_mode()
    def _exec_embed(self, plan: Dict[str, Any]) -> torch.Tensor:
        """Dense forward WITHOUT touching the KV cache: returns mean-pooled,
        L2-normalized final hidden states [b, hidden] (the v1/embeddings
        serve path; reference delegates this to vLLM's pooling stack,
        preprocess_service.py:632-1095)."""
        prompts = plan["prompts"]
        b = len(prompts)
        lens = [len(p) for p in prompts]
        smax = max(lens)
        dev = self.device
        tokens = torch.zeros(b, smax, dtype=torch.long)
        positions = torch.zeros(b, smax, dtype=torch.int32)
        for i in range(b):
            tokens[i, :lens[i]] = torch.tensor(prompts[i], dtype=torch.long)
            positions[i, :lens[i]] = torch.arange(lens[i], dtype=torch.int32)
        attn_ctx = {
            "mode": "prefill", "batch": b, "seq": smax,
            "seq_lens": torch.tensor(lens, dtype=torch.int32, device=dev),
        }
        hidden = self.model(
            tokens.view(-1).to(dev), positions.view(-1).to(dev),
            kv_caches=None, attn_ctx=attn_ctx,
            return_hidden=True).view(b, smax, -1).float()
        mask = (torch.arange(smax, device=dev)[None, :]
                < torch.tensor(lens, device=dev)[:, None]).unsqueeze(-1)
        # where(), not multiply: pad rows hold garbage (possibly NaN/inf
        # from fully-masked attention) and NaN * 0 is NaN
        pooled = torch.where(mask, hidden, 0.0).sum(1) \
            / mask.sum(1).clamp(min=1)
        if plan.get("normalize", True):
            pooled = torch.nn.functional.normalize(pooled, dim=-1)
        return pooled

    def _embed_sync(self, plan: Dict[str, Any]) -> List[List[float]]:
        """Broadcast + dense forward under the exec lock: never concurrent
        with step() (graph capture / TP plan ordering) and never on the
        event-loop thread (a dense forward would stall every endpoint)."""
        with self._exec_lock:
            self._tp_broadcast(plan)
            return self._exec_embed(plan).cpu().tolist()

    async def embed_batch(self, texts: List[str]) -> List[List[float]]:
        if self.model is None:
            raise RuntimeError("LLM engine not started")
        prompts = [self.tokenizer.encode(t)[:self.cfg.max_model_len]
                   for t in texts]
        plan = {"mode": "embed", "prompts": prompts}
        return await asyncio.to_thread(self._embed_sync, plan)

    def _preempt_one(self) -> bool:
        """KV pressure relief: evict the newest running sequence back to the
        waiting queue (vLLM-style recompute preemption -- its prompt plus
        generated tokens re-prefill when pages free up)."""
        candidates = [s for s in self.running if not s.finished]
        if len(candidates) <= 1:
            return False
        victim = max(candidates, key=lambda s: s.created)
        self.running.remove(victim)
        self._free_blocks(victim)
        victim.prompt_ids = victim.prompt_ids + victim.output_ids
        victim.output_ids = []
        self.waiting.insert(0, victim)
        self.stats["preemptions"] = self.stats.get("preemptions", 0) + 1
        return True

    def _decode(self, seqs: List[Sequence]) -> None:
        self.stats["decode_batches"] += 1
        bs_cfg = self.cfg.block_size
        # grow block tables for the token being generated; under KV pressure
        # preempt the newest sequences instead of failing the whole engine
        for s in list(seqs):
            pos = len(s) - 1  # position of the last generated token
            if pos // bs_cfg >= len(s.blocks):
                while self.allocator.available < 1:
                    if not self._preempt_one():
                        raise RuntimeError(
                            "KV cache exhausted with a single sequence -- "
                            "raise num_kv_blocks / gpu_memory_fraction")
                    if s not in self.running:  # we evicted s itself
                        break
                if s not in self.running:
                    seqs.remove(s)
                    continue
                s.blocks.extend(self.allocator.alloc(1))
        # a preemption victim other than ``s`` stays in ``seqs`` until its
        # own iteration, where blocks == [] forces it into the growth branch
        # above and out of the batch -- make that invariant explicit so the
        # plan below can never index a freed block list
        seqs[:] = [s for s in seqs if s in self.running]
        if not seqs:
            return
        plan = {
            "mode": "decode",
            "tokens": [s.output_ids[-1] for s in seqs],
            "positions": [len(s) - 1 for s in seqs],
            "slots": [self._slot(s, len(s) - 1) for s in seqs],
            "seq_lens": [len(s) for s in seqs],
            "blocks": [self._block_table(s) for s in seqs],
            "sample": self._sample_spec(seqs),
        }
        if self.lora_bank is not None:
            plan["lora"] = [s.lora_idx for s in seqs]
        self._tp_broadcast(plan)
        logits = self._exec_decode(plan)
        self._sample_and_emit(seqs, logits, sample=plan["sample"])

    def _use_microbatch(self, b: int) -> bool:
        """TP decode microbatch pipelining (comm/compute overlap): split
        the decode batch in two and overlap each half's all-reduces with
        the other half's compute (model.forward_pipelined). OFF by default
        -- correctness is gloo-verified (tests/helpers/tp_check.py) but the
        schedule is unmeasured on multi-GPU hardware, and it bypasses the
        decode hipGraphs (the eager pipeline re-pays launch overhead);
        first 8-GPU window: measure CMLS_TP_MICROBATCH=1 vs graphs."""
        return (getattr(self, "tp_size", 1) > 1 and b >= 2
                and os.environ.get("CMLS_TP_MICROBATCH", "0") == "1")

    @torch.inference_mode()
    def _exec_decode(self, plan: Dict[str, Any]) -> torch.Tensor:
        b = len(plan["tokens"])
        if self._use_microbatch(b):
            return self._exec_decode_microbatch(plan)
        if self._use_decode_graphs():
            return self._exec_decode_graph(plan)
        dev = self.device
        tokens = torch.tensor(plan["tokens"], dtype=torch.long, device=dev)
        positions = torch.tensor(plan["positions"], dtype=torch.int32,
                                 device=dev)
        slot_map = torch.tensor(plan["slots"], dtype=torch.int32, device=dev)
        max_blocks = max(len(bl) for bl in plan["blocks"])
        btab = torch.zeros(b, max_blocks, dtype=torch.int32)
        for i, bl in enumerate(plan["blocks"]):
            btab[i, :len(bl)] = torch.tensor(bl, dtype=torch.int32)
        attn_ctx = {
            "mode": "decode",
            "seq_lens": torch.tensor(plan["seq_lens"], dtype=torch.int32,
                                     device=dev),
            "block_table": btab.to(dev),
            "slot_mapping": slot_map,
        }
        if "lora" in plan:
            self._lora_ctx(attn_ctx, plan["lora"])
        return self.model(tokens, positions, kv_caches=self.kv_caches,
                          attn_ctx=attn_ctx, last_token_idx=None,
                          gather_logits=False)

    @torch.inference_mode()
    def _exec_decode_microbatch(self, plan: Dict[str, Any]) -> torch.Tensor:
        """Split the decode plan into two row-halves and run them through
        model.forward_pipelined. The split point is derived from the plan
        (identical on every rank), so all ranks issue the pipeline's
        collectives in the same order."""
        dev = self.device
        b = len(plan["tokens"])
        mid = b // 2
        parts = []
        for lo, hi in ((0, mid), (mid, b)):
            rows = range(lo, hi)
            tokens = torch.tensor([plan["tokens"][i] for i in rows],
                                  dtype=torch.long, device=dev)
            positions = torch.tensor([plan["positions"][i] for i in rows],
                                     dtype=torch.int32, device=dev)
            slot_map = torch.tensor([plan["slots"][i] for i in rows],
                                    dtype=torch.int32, device=dev)
            blocks = [plan["blocks"][i] for i in rows]
            max_blocks = max(len(bl) for bl in blocks)
            btab = torch.zeros(hi - lo, max_blocks, dtype=torch.int32)
            for i, bl in enumerate(blocks):
                btab[i, :len(bl)] = torch.tensor(bl, dtype=torch.int32)
            attn_ctx = {
                "mode": "decode",
                "seq_lens": torch.tensor(
                    [plan["seq_lens"][i] for i in rows],
                    dtype=torch.int32, device=dev),
                "block_table": btab.to(dev),
                "slot_mapping": slot_map,
            }
            parts.append((tokens, positions, attn_ctx))
        return self.model.forward_pipelined(parts, self.kv_caches)

    # -------------------- speculative decoding (ngram) ---------------- #
    # Prompt-lookup speculation (vLLM's "ngram" method): propose the K
    # tokens that followed the most recent earlier occurrence of the
    # context's trailing N-gram, verify all of them in ONE multi-token
    # forward (the chunked-prefill paged-attention path), and accept the
    # longest prefix that matches greedy argmax -- exact greedy output, up
    # to K+1 tokens per step. Rollback is free: KV slots are addressed by
    # sequence position, so a rejected position's K/V is overwritten when
    # that position is really generated (and never attended before then,
    # kv_lens only counts committed tokens).
    def _spec_tokens(self) -> int:
        spec = self.cfg.speculative
        if not spec:
            return 0
        if str(spec.get("method", "ngram")) != "ngram":
            raise ValueError("unsupported speculative method '{}' (have: "
                             "ngram)".format(spec.get("method")))
        return max(int(spec.get("num_spec_tokens", 4)), 0)

    def _ngram_propose(self, s: Sequence, k: int) -> List[int]:
        n = max(int((self.cfg.speculative or {}).get("ngram", 2)), 1)
        ctx = s.prompt_ids + s.output_ids
        if len(ctx) <= n:
            return []
        tail = ctx[-n:]
        # most recent earlier occurrence of the trailing n-gram
        for m in range(len(ctx) - n - 1, -1, -1):
            if ctx[m:m + n] == tail:
                return list(ctx[m + n:m + n + k])
        return []

    def _decode_spec(self, seqs: List[Sequence], k: int) -> None:
        assert getattr(self, "tp_size", 1) <= 1
        bs = self.cfg.block_size
        # base-token block growth: identical contract to _decode (preempts
        # under KV pressure; evicted victims leave the batch)
        for s in list(seqs):
            pos = len(s) - 1
            if pos // bs >= len(s.blocks):
                while self.allocator.available < 1:
                    if not self._preempt_one():
                        raise RuntimeError(
                            "KV cache exhausted with a single sequence -- "
                            "raise num_kv_blocks / gpu_memory_fraction")
                    if s not in self.running:
                        break
                if s not in self.running:
                    seqs.remove(s)
                    continue
                s.blocks.extend(self.allocator.alloc(1))
        seqs[:] = [s for s in seqs if s in self.running]
        if not seqs:
            return

        proposals: List[List[int]] = []
        for s in seqs:
            cap = min(k,
                      s.params.max_tokens - s.generated - 1,
                      self.cfg.max_model_len - len(s) - 1)
            # backoff: a sequence whose last 4 proposals were all rejected
            # is generating non-repetitive text -- stop paying the
            # multi-token verify for it, retry every 32 tokens in case the
            # output becomes structured again
            if s.spec_misses >= 4 and s.generated % 32 != 0:
                cap = 0
            prop = self._ngram_propose(s, cap) if cap > 0 else []
            # proposal tokens occupy positions len(s)..len(s)+p-1: extend
            # the block table opportunistically, trimming to what the
            # allocator has (never preempt for speculation)
            while prop:
                need = (len(s) + len(prop) + bs - 1) // bs - len(s.blocks)
                if need <= 0:
                    break
                if need > self.allocator.available:
                    prop = prop[:-1]
                    continue
                s.blocks.extend(self.allocator.alloc(need))
                break
            proposals.append(prop)

        if not any(proposals):
            # nothing to verify: the plain decode path (hipGraph-replayed
            # on GPU) is strictly faster than a 1-token chunk forward
            self._decode(seqs)
            return

        self.stats["decode_batches"] += 1
        plan = {
            "mode": "spec",
            "tokens": [[s.output_ids[-1]] + prop
                       for s, prop in zip(seqs, proposals)],
            "starts": [len(s) - 1 for s in seqs],
            "kv_lens": [len(s) + len(prop)
                        for s, prop in zip(seqs, proposals)],
            "slots": [[self._slot(s, p)
                       for p in range(len(s) - 1, len(s) + len(prop))]
                      for s, prop in zip(seqs, proposals)],
            "blocks": [self._block_table(s) for s in seqs],
        }
        if self.lora_bank is not None:
            plan["lora"] = [s.lora_idx for s in seqs]
        logits = self._exec_spec(plan)

        off = 0
        argmax = logits.argmax(dim=-1).cpu()
        for s, prop in zip(seqs, proposals):
            n = 1 + len(prop)
            rows = argmax[off:off + n]
            off += n
            toks: List[int] = []
            for j in range(n):
                toks.append(int(rows[j]))
                if not (j < len(prop) and toks[-1] == prop[j]):
                    break
            self.stats["spec_proposed"] = (
                self.stats.get("spec_proposed", 0) + len(prop))
            self.stats["spec_accepted"] = (
                self.stats.get("spec_accepted", 0) + len(toks) - 1)
            if prop:
                s.spec_misses = 0 if len(toks) > 1 else s.spec_misses + 1
            self._emit_tokens(s, toks)

    @torch.inference_mode()
    def _exec_spec(self, plan: Dict[str, Any]) -> torch.Tensor:
        """Multi-token verification forward: the chunk layout (padded
        [b, smax] batch, paged attention over each sequence's committed
        history + in-flight proposal) but gathering logits at EVERY real
        row, concatenated in batch order."""
        dev = self.device
        b = len(plan["tokens"])
        lens = [len(t) for t in plan["tokens"]]
        smax = max(lens)
        tokens = torch.zeros(b, smax, dtype=torch.long)
        positions = torch.zeros(b, smax, dtype=torch.int32)
        slot_map = torch.full((b, smax), -1, dtype=torch.int32)
        for i in range(b):
            n = lens[i]
            tokens[i, :n] = torch.tensor(plan["tokens"][i], dtype=torch.long)
            positions[i, :n] = torch.arange(
                plan["starts"][i], plan["starts"][i] + n, dtype=torch.int32)
            slot_map[i, :n] = torch.tensor(plan["slots"][i],
                                           dtype=torch.int32)
        max_blocks = max(len(bl) for bl in plan["blocks"])
        btab = torch.zeros(b, max_blocks, dtype=torch.int32)
        for i, bl in enumerate(plan["blocks"]):
            btab[i, :len(bl)] = torch.tensor(bl, dtype=torch.int32)
        attn_ctx = {
            "mode": "prefill_paged", "batch": b, "seq": smax,
            "kv_lens": torch.tensor(plan["kv_lens"], dtype=torch.int32,
                                    device=dev),
            "q_lens": torch.tensor(lens, dtype=torch.int32, device=dev),
            "block_table": btab.to(dev),
            "slot_mapping": slot_map.view(-1).to(dev),
        }
        if "lora" in plan:
            self._lora_ctx(attn_ctx, plan["lora"], lens, smax)
        rows = [i * smax + j for i in range(b) for j in range(lens[i])]
        last_idx = torch.tensor(rows, dtype=torch.long, device=dev)
        return self.model(tokens.view(-1).to(dev),
                          positions.view(-1).to(dev),
                          kv_caches=self.kv_caches, attn_ctx=attn_ctx,
                          last_token_idx=last_idx, gather_logits=False)

    # -------------------- decode hipGraph capture --------------------- #
    # A llama-8B decode step dispatches ~350 kernels from Python; at B=64
    # the weight streaming itself is only ~2.5 ms, so the step is
    # launch/dispatch bound. Capturing one hipGraph per batch bucket
    # (padded rows: slot=-1 so the KV scatter skips them, block_table=0 /
    # seq_len=1 so the attention read is bounded) replays the whole step
    # as a single launch. vLLM uses the same strategy on its decode path.
    def _use_decode_graphs(self) -> bool:
        # TP: RCCL all-reduces ARE capturable in hipGraphs (the tp_serve
        # launcher sets TORCH_NCCL_ASYNC_ERROR_HANDLING=0, required for
        # collective capture); CMLS_TP_GRAPHS=0 is the kill switch
        if (getattr(self, "tp_size", 1) > 1
                and os.environ.get("CMLS_TP_GRAPHS", "1") == "0"):
            return False
        return (self.cfg.decode_graphs
                and self.device.type == "cuda"
                and os.environ.get("CMLS_LLM_GRAPHS", "1") != "0")

    def _decode_bucket(self, b: int) -> int:
        for cand in self._decode_buckets:
            if cand >= b:
                return cand
        return self._decode_buckets[-1]

    def _graph_entry(self, bucket: int) -> Dict[str, Any]:
        entry = self._decode_graphs.get(bucket)
        if entry is not None:
            return entry
        dev = self.device
        mb = (self.cfg.max_model_len + self.cfg.block_size - 1) \
            // self.cfg.block_size
        static = {
            "tokens": torch.zeros(bucket, dtype=torch.long, device=dev),
            "positions": torch.zeros(bucket, dtype=torch.int32, device=dev),
            "slots": torch.full((bucket,), -1, dtype=torch.int32, device=dev),
            "seq_lens": torch.ones(bucket, dtype=torch.int32, device=dev),
            "block_table": torch.zeros(bucket, mb, dtype=torch.int32,
                                       device=dev),
        }
        attn_ctx = {"mode": "decode", "seq_lens": static["seq_lens"],
                    "block_table": static["block_table"],
                    "slot_mapping": static["slots"]}
        if self.lora_bank is not None:
            # one graph per bucket whatever the adapter mix: the captured
            # LoRA kernels read this buffer; padded rows stay -1 (skipped)
            static["lora_idx"] = torch.full((bucket,), -1, dtype=torch.int32,
                                            device=dev)
            attn_ctx["lora"] = (self.lora_bank, static["lora_idx"])

        def fwd():
            return self.model(static["tokens"], static["positions"],
                              kv_caches=self.kv_caches, attn_ctx=attn_ctx,
                              last_token_idx=None, gather_logits=False)

        # warm up on a side stream (allocator + kernels settle), capture on
        # the current stream; all graphs share one memory pool
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                fwd()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        if self._graph_pool is None:
            with torch.cuda.graph(graph):
                static["logits"] = fwd()
            self._graph_pool = graph.pool()
        else:
            with torch.cuda.graph(graph, pool=self._graph_pool):
                static["logits"] = fwd()
        entry = {"graph": graph, **static}
        self._decode_graphs[bucket] = entry
        self.stats["graph_captures"] += 1
        return entry

    def _exec_decode_graph(self, plan: Dict[str, Any]) -> torch.Tensor:
        b = len(plan["tokens"])
        bucket = self._decode_bucket(b)
        entry = self._graph_entry(bucket)
        # stage this step's inputs in pinned host memory, one async H2D per
        # buffer into the graph's static tensors
        pin = self._decode_pin.get(bucket)
        mb = entry["block_table"].shape[1]
        if pin is None:
            pin = {
                "tokens": torch.zeros(bucket, dtype=torch.long,
                                      pin_memory=True),
                "positions": torch.zeros(bucket, dtype=torch.int32,
                                         pin_memory=True),
                "slots": torch.empty(bucket, dtype=torch.int32,
                                     pin_memory=True),
                "seq_lens": torch.ones(bucket, dtype=torch.int32,
                                       pin_memory=True),
                "block_table": torch.zeros(bucket, mb, dtype=torch.int32,
                                           pin_memory=True),
            }
            self._decode_pin[bucket] = pin
        pin["tokens"][:b] = torch.tensor(plan["tokens"], dtype=torch.long)
        pin["tokens"][b:] = 0
        pin["positions"][:b] = torch.tensor(plan["positions"],
                                            dtype=torch.int32)
        pin["positions"][b:] = 0
        pin["slots"][:b] = torch.tensor(plan["slots"], dtype=torch.int32)
        pin["slots"][b:] = -1  # padded rows: KV scatter kernel skips slot<0
        pin["seq_lens"][:b] = torch.tensor(plan["seq_lens"],
                                           dtype=torch.int32)
        pin["seq_lens"][b:] = 1
        bt = pin["block_table"]
        bt.zero_()
        for i, bl in enumerate(plan["blocks"]):
            bt[i, :len(bl)] = torch.tensor(bl, dtype=torch.int32)
        for k in ("tokens", "positions", "slots", "seq_lens", "block_table"):
            entry[k].copy_(pin[k], non_blocking=True)
        if "lora" in plan:
            if "lora_idx" not in pin:
                pin["lora_idx"] = torch.empty(bucket, dtype=torch.int32,
                                              pin_memory=True)
            pin["lora_idx"][:b] = torch.tensor(plan["lora"],
                                               dtype=torch.int32)
            pin["lora_idx"][b:] = -1  # padded rows: LoRA kernels skip idx<0
            entry["lora_idx"].copy_(pin["lora_idx"], non_blocking=True)
        entry["graph"].replay()
        self.stats["graph_replays"] += 1
        return entry["logits"][:b]

    # ------------------------------------------------------------------ #
    # tensor-parallel coordination (rank 0 schedules, workers follow)
    # ------------------------------------------------------------------ #
    def _tp_broadcast(self, plan: Optional[Dict[str, Any]]) -> None:
        """ONE fixed-layout int32 tensor broadcast per step (RCCL on GPU).
        Round 1 used broadcast_object_list -- pickle + CPU sync per decode
        step, fatal for a TP=8 latency budget; plans that overflow the fixed
        buffer (rare giant embed batches) fall back to the object path."""
        if getattr(self, "tp_size", 1) <= 1 or self.tp_rank != 0:
            return
        import torch.distributed as dist

        buf = self._plan_codec.encode(plan)
        if buf is None:
            dist.broadcast(self._plan_codec.mark_object(), src=0)
            dist.broadcast_object_list([plan], src=0)
        else:
            dist.broadcast(buf, src=0)

    def _tp_receive(self) -> Dict[str, Any]:
        import torch.distributed as dist

        dist.broadcast(self._plan_codec.buf, src=0)
        plan = self._plan_codec.decode(self._plan_codec.buf)
        if plan is None:  # object fallback
            box = [None]
            dist.broadcast_object_list(box, src=0)
            plan = box[0] or {"mode": "stop"}
        return plan

    def run_tp_worker(self) -> None:
        """Worker-rank loop: execute rank 0's step plans until shutdown.

        The model's row-parallel all-reduces are per-layer sync points; the
        sampling collectives (packed-argmax all-reduce / rank-0 gather) make
        every rank participate in token selection, so no rank ever
        materializes full-vocab logits."""
        assert self.tp_size > 1 and self.tp_rank != 0
        while True:
            plan = self._tp_receive()
            mode = plan.get("mode")
            if mode == "stop":
                return
            if mode == "prefill":
                logits = self._exec_prefill(plan)
            elif mode == "chunk":
                logits = self._exec_chunk(plan)
            elif mode == "embed":
                self._exec_embed(plan)
                continue
            else:
                logits = self._exec_decode(plan)
            if plan.get("sample"):
                self._tp_sample_rows(logits, plan["sample"])

    def _tp_sample_rows(self, logits: torch.Tensor, sample) -> torch.Tensor:
        """Collective sampling over vocab-sharded logits; every rank calls
        this with the identical ``sample`` row list (from the plan), so the
        collectives line up. Returns next token ids (valid on rank 0; the
        argmax/gumbel paths are valid on every rank)."""
        from ...parallel import tp as tp_mod

        groups: Dict[tuple, List[int]] = {}
        for i, row in enumerate(sample):
            groups.setdefault(tuple(row), []).append(i)
        next_ids = torch.zeros(len(sample), dtype=torch.long)
        voff = self.tp_rank * logits.shape[-1]
        for (temp, top_k, top_p, seed), idxs in groups.items():
            rows = logits[idxs]
            if top_k > 0 or top_p < 1.0:
                # full distribution needed: gather these rows to rank 0
                full = tp_mod.gather_rows_to_rank0(rows)
                if self.tp_rank == 0:
                    gen = torch.Generator(device=full.device)
                    gen.manual_seed(int(seed) & 0x7FFFFFFF)
                    sampled = ops.sample_top_k_top_p(
                        full, temperature=temp, top_k=top_k, top_p=top_p,
                        generator=gen)
                else:
                    sampled = torch.zeros(len(idxs), dtype=torch.long)
            elif temp == 0.0:
                sampled = tp_mod.argmax_sharded(rows, voff)
            else:
                sampled = tp_mod.sample_gumbel_sharded(
                    rows, voff, temp, [seed])
            next_ids[idxs] = sampled.to("cpu", dtype=torch.long)
        return next_ids

    def tp_shutdown(self) -> None:
        if getattr(self, "tp_size", 1) > 1 and self.tp_rank == 0:
            # serialize with any in-flight step/embed broadcast so worker
            # ranks never see "stop" interleaved inside another plan
            with self._exec_lock:
                self._tp_broadcast({"mode": "stop"})

    def _apply_penalties(self, logits: torch.Tensor,
                         seqs: List[Sequence]) -> torch.Tensor:
        """OpenAI presence/frequency penalties (output tokens) + CTRL-style
        repetition penalty (prompt+output) + min_tokens eos masking (like
        vLLM: the eos/stop ids are banned from sampling until min_tokens,
        not post-filtered). Applied per requesting row only; the tensor is
        cloned first because decode-graph logits are static replay buffers
        that must never be mutated."""
        need = [i for i, s in enumerate(seqs)
                if s.params.has_penalties()
                or s.params.min_tokens > s.generated]
        if not need:
            return logits
        V = logits.shape[-1]
        dev = logits.device
        logits = logits.clone()
        for i in need:
            s = seqs[i]
            p = s.params
            row = logits[i].float()
            if p.min_tokens > s.generated:
                ban = list(p.stop_token_ids)
                if not p.ignore_eos:
                    ban.append(self.tokenizer.eos_id)
                ban = [t for t in ban if 0 <= t < V]
                if ban:
                    row[torch.tensor(ban, dtype=torch.long,
                                     device=dev)] = float("-inf")
            if p.repetition_penalty != 1.0:
                ctx = [t for t in dict.fromkeys(s.prompt_ids + s.output_ids)
                       if 0 <= t < V]
                if ctx:
                    idx = torch.tensor(ctx, dtype=torch.long, device=dev)
                    vals = row[idx]
                    row[idx] = torch.where(
                        vals > 0, vals / p.repetition_penalty,
                        vals * p.repetition_penalty)
            if s.output_ids and (p.presence_penalty or p.frequency_penalty):
                out = torch.tensor(
                    [t for t in s.output_ids if 0 <= t < V],
                    dtype=torch.long, device=dev)
                counts = torch.bincount(out, minlength=V).to(row.dtype)
                row -= p.frequency_penalty * counts
                row -= p.presence_penalty * (counts > 0).to(row.dtype)
            logits[i] = row.to(logits.dtype)
        return logits

    def _hit_stop_string(self, s: Sequence) -> bool:
        """OpenAI 'stop' strings: decode a bounded tail window of the output
        after each token and look for any stop sequence (the reference's
        vLLM path matches decoded text the same way). The final text is
        truncated at the stop by _truncate_at_stop()."""
        window = min(len(s.output_ids), 16)
        tail = self.tokenizer.decode(s.output_ids[-window:])
        return any(st in tail for st in s.params.stop)

    @staticmethod
    def _truncate_at_stop(text: str, params: SamplingParams,
                          reason: Optional[str]) -> str:
        if reason != "stop" or not params.stop:
            return text
        cut = len(text)
        for st in params.stop:
            idx = text.find(st)
            if idx >= 0:
                cut = min(cut, idx)
        return text[:cut]

    def _sample_and_emit(self, seqs: List[Sequence], logits: torch.Tensor,
                         sample: Optional[List[tuple]] = None) -> None:
        if getattr(self, "tp_size", 1) > 1:
            # collective sampling over vocab shards (workers run the same
            # call from run_tp_worker with the identical plan spec)
            next_ids = self._tp_sample_rows(
                logits, sample or self._sample_spec(seqs))
        elif self.mask_bank is not None \
                and any(s.guided is not None for s in seqs):
            self._sample_guided(seqs, logits)
            return
        else:
            logits, next_ids = self._sample_grouped(seqs, logits)
        self._emit_sampled(seqs, next_ids, logits)

    def _sample_grouped(self, seqs: List[Sequence], logits: torch.Tensor):
        """Penalties, then one sampler launch per group of rows with
        identical sampling params -> (post-penalty logits, next ids)."""
        logits = self._apply_penalties(logits, seqs)
        # group rows by identical sampling params for batched kernels
        # (a request-level seed gets its own group + generator)
        groups: Dict[tuple, List[int]] = {}
        for i, s in enumerate(seqs):
            key = (s.params.temperature, s.params.top_k, s.params.top_p,
                   s.params.seed)
            groups.setdefault(key, []).append(i)
        next_ids = torch.empty(len(seqs), dtype=torch.long)
        for (temp, top_k, top_p, seed), idxs in groups.items():
            rows = logits[idxs] if len(idxs) < len(seqs) else logits
            gen = None
            if seed is not None and temp != 0.0:
                s0 = seqs[idxs[0]]
                gen = torch.Generator(device=logits.device)
                gen.manual_seed((seed + s0.generated) & 0x7FFFFFFF)
            sampled = ops.sample_top_k_top_p(
                rows, temperature=temp, top_k=top_k, top_p=top_p,
                generator=gen)
            next_ids[idxs] = sampled.cpu()
        return logits, next_ids

    def _sample_guided(self, seqs: List[Sequence],
                       logits: torch.Tensor) -> None:
        """A step with at least one guided row (TP=1). Plain rows (no
        top-k/top-p, penalties, logprobs or min_tokens ban) -- guided or
        not -- go through ONE fused mask+draw launch with per-row
        temperature and seed; the others are masked out of place and then
        take the usual penalties -> grouped sampler -> logprobs flow, so
        the mask applies before the penalties and logprobs are those of
        the masked distribution."""
        bank = self.mask_bank
        bank.begin_step()
        slots: List[int] = []
        for s in seqs:
            if s.guided is None:
                slots.append(-1)
            elif s.guided.num_allowed() == 0:
                slots.append(-2)  # dead end: not sampled at all
            else:
                slots.append(bank.acquire(s.guided.key, s.guided.mask_words))
        fused, rest = [], []
        for i, s in enumerate(seqs):
            p = s.params
            if slots[i] == -2:
                self._finish_dead_end(s)
            elif (p.top_k > 0 or p.top_p < 1.0 or p.has_penalties()
                  or p.logprobs is not None or p.min_tokens > s.generated):
                rest.append(i)
            else:
                fused.append(i)
        dev = logits.device

        def rows_of(idxs):
            return logits if len(idxs) == len(seqs) else logits[idxs]

        fused_ids = rest_ids = rest_logits = None
        if fused:
            draws = torch.randint(0, 2**31 - 1, (len(fused),)).tolist()
            seeds = [(seqs[i].params.seed + seqs[i].generated) & 0x7FFFFFFF
                     if seqs[i].params.seed is not None else draws[j]
                     for j, i in enumerate(fused)]
            fused_ids = ops.sample_token_bitmask(
                rows_of(fused), bank.bank,
                torch.tensor([slots[i] for i in fused], dtype=torch.int32,
                             device=dev),
                torch.tensor([seqs[i].params.temperature for i in fused],
                             dtype=torch.float32, device=dev),
                torch.tensor(seeds, dtype=torch.int32, device=dev))
        if rest:
            masked = ops.apply_token_bitmask(
                rows_of(rest), bank.bank,
                torch.tensor([slots[i] for i in rest], dtype=torch.int32,
                             device=dev))
            rest_logits, rest_ids = self._sample_grouped(
                [seqs[i] for i in rest], masked)
        if fused:
            fused_ids = fused_ids.cpu()
            live = []
            for j, i in enumerate(fused):
                if int(fused_ids[j]) < 0:  # nothing finite to draw from
                    self._finish_dead_end(seqs[i])
                else:
                    live.append(j)
            self._emit_sampled([seqs[fused[j]] for j in live],
                               fused_ids[live], None)
        if rest:
            self._emit_sampled([seqs[i] for i in rest], rest_ids,
                               rest_logits)

    def _emit_sampled(self, seqs: List[Sequence], next_ids: torch.Tensor,
                      logits: Optional[torch.Tensor]) -> None:
        for i, s in enumerate(seqs):
            tok = int(next_ids[i])
            extra = None
            if s.params.logprobs is not None \
                    and getattr(self, "tp_size", 1) <= 1:
                # logprobs of the ACTUAL sampling distribution (post-
                # penalty logits), like the reference's vLLM path
                row = torch.log_softmax(logits[i].float(), dim=-1)
                e = {"logprob": float(row[tok])}
                k = s.params.logprobs
                if k:
                    topv, topi = row.topk(k)
                    e["top_logprobs"] = {
                        int(t): float(v)
                        for v, t in zip(topv.tolist(), topi.tolist())}
                extra = [e]
            self._emit_tokens(s, [tok], extras=extra)

    def _guided_advance(self, s: Sequence, tok: int) -> bool:
        """Move a guided sequence's DFA past ``tok``; True when the output
        is complete -- accepting with nothing but eos left to say -- or the
        grammar dead-ends, so no further step is spent on it."""
        g = s.guided
        g.advance(tok)
        if g.num_continuations() > 0:
            return False
        if not g.accepting():
            self._note_dead_end(s)
        return True

    def _emit_tokens(self, s: Sequence, toks: List[int],
                     extras: Optional[List[Optional[dict]]] = None) -> None:
        """Append generated tokens to a sequence, applying the stop/eos/
        length rules per token (emission halts at the first finish -- extra
        speculative tokens past a stop are dropped)."""
        eos = self.tokenizer.eos_id
        now = time.time()
        for ti, tok in enumerate(toks):
            if s.finished:
                break
            s.output_ids.append(tok)
            s.generated += 1
            if s.first_token_time is None:
                s.first_token_time = now
            self.stats["generated_tokens"] += 1
            finished = False
            reason = None
            if (not s.params.ignore_eos and tok == eos) \
                    or tok in s.params.stop_token_ids:
                finished, reason = True, "stop"
            elif s.guided is not None and self._guided_advance(s, tok):
                finished, reason = True, "stop"
            elif s.params.stop and self._hit_stop_string(s):
                finished, reason = True, "stop"
            elif s.generated >= s.params.max_tokens:
                finished, reason = True, "length"
            elif len(s) >= self.cfg.max_model_len:
                finished, reason = True, "length"
            s.finished = finished
            s.finish_reason = reason
            # streamed text = the DELTA of the cumulative decode, not a
            # per-token decode: a multi-byte character split across BPE
            # tokens would otherwise stream as replacement chars (vLLM's
            # incremental detokenization does the same). An incomplete
            # UTF-8 tail is held back until the next token completes it.
            full = self.tokenizer.decode(s.output_ids)
            if len(full) < s.text_sent:  # non-prefix-stable decode: resync
                s.text_sent = len(full)
            delta = full[s.text_sent:]
            if not finished and delta.endswith("�"):
                delta = delta[:-1]
            s.text_sent += len(delta)
            item = {
                "token_ids": [tok],
                "text": delta,
                "finished": finished,
                "finish_reason": reason,
            }
            if extras is not None and ti < len(extras) and extras[ti]:
                item.update(extras[ti])
            s.stream.put_nowait(item)

    # ------------------------------------------------------------------ #
    # OpenAI-compatible handlers (route /serve/openai/v1/*)
    # ------------------------------------------------------------------ #
    def _chat_prompt(self, messages: List[Dict[str, str]]) -> str:
        if getattr(self.tokenizer, "is_llama3", False):
            # real llama-3 chat template (the tokenizer carries the
            # header-id special tokens, so they encode to their single ids)
            parts = ["<|begin_of_text|>"]
            for m in messages:
                parts.append("<|start_header_id|>{}<|end_header_id|>\n\n{}"
                             "<|eot_id|>".format(m.get("role", "user"),
                                                 m.get("content", "")))
            parts.append("<|start_header_id|>assistant<|end_header_id|>\n\n")
            return "".join(parts)
        if getattr(self.tokenizer, "is_chatml", False):
            # ChatML (Qwen2 family): <|im_start|>role\ncontent<|im_end|>
            parts = []
            for m in messages:
                parts.append("<|im_start|>{}\n{}<|im_end|>\n".format(
                    m.get("role", "user"), m.get("content", "")))
            parts.append("<|im_start|>assistant\n")
            return "".join(parts)
        # synthetic fallback (byte tokenizer / random-init serving)
        parts = []
        for m in messages:
            parts.append("<|{}|>\n{}".format(m.get("role", "user"),
                                             m.get("content", "")))
        parts.append("<|assistant|>\n")
        return "\n".join(parts)

    @staticmethod
    def _n_choices(body: Dict[str, Any]) -> int:
        n = body.get("n", 1)
        try:
            n = int(n) if n is not None else 1
        except (TypeError, ValueError, OverflowError):
            raise ValueError("'n' must be an integer")
        if not (1 <= n <= 16):
            raise ValueError("'n' must be in [1, 16], got {}".format(n))
        if n > 1 and body.get("stream"):
            raise ValueError("streaming with n > 1 is not supported; "
                             "request the choices without 'stream'")
        bo = body.get("best_of")
        try:
            bo = int(bo) if bo is not None else None
        except (TypeError, ValueError, OverflowError):
            raise ValueError("'best_of' must be an integer")
        if bo is not None and bo != n:
            # OpenAI deprecated best_of; silently ignoring it would change
            # semantics (it implies server-side reranking)
            raise ValueError(
                "'best_of' != n is not supported (best_of reranking is "
                "deprecated by OpenAI); request n choices and pick "
                "client-side")
        return n

    def _choice_params(self, body: Dict[str, Any], n: int
                       ) -> List[SamplingParams]:
        """One SamplingParams per choice; an explicit request seed is
        offset per choice so the n completions differ (same OpenAI
        semantics: n identical greedy choices are expected)."""
        out = []
        for i in range(n):
            p = SamplingParams.from_request(
                body, guided=self.cfg.guided_decoding)
            if p.guided is not None and i == 0:
                # compile now (LRU-cached for add_request): a grammar error
                # must 422 before a streaming response has started
                self._guided_state(p)
            if p.seed is not None:
                p.seed = (p.seed + 7919 * i) & 0x7FFFFFFF
            out.append(p)
        return out

    async def openai_chat_completions(self, body: Dict[str, Any],
                                      model_name: str):
        messages = body.get("messages") or []
        prompt = self._chat_prompt(messages)
        n = self._n_choices(body)
        params = self._choice_params(body, n)
        rid = "chatcmpl-" + uuid.uuid4().hex[:24]
        # "model" naming a configured LoRA adapter routes to it (and is
        # echoed); any other value serves the base model
        lora_idx = self._resolve_lora(body.get("model"))
        if lora_idx >= 0:
            model_name = body["model"]
        if body.get("stream"):
            opts = body.get("stream_options") or {}
            return self._sse_stream(prompt, params[0], rid, model_name,
                                    chat=True,
                                    include_usage=bool(
                                        opts.get("include_usage")),
                                    lora_idx=lora_idx)
        results = await asyncio.gather(
            *[self._collect(prompt, p, lora_idx) for p in params])
        nprompt = results[0][3]
        ntok = sum(r[2] for r in results)
        choices = []
        for i, r in enumerate(results):
            choice = {"index": i,
                      "message": {"role": "assistant", "content": r[0]},
                      "finish_reason": r[1]}
            if params[i].logprobs is not None:
                choice["logprobs"] = self._chat_logprobs(r[4])
            choices.append(choice)
        return {
            "id": rid, "object": "chat.completion", "created": int(time.time()),
            "model": model_name,
            "choices": choices,
            "usage": {"prompt_tokens": nprompt, "completion_tokens": ntok,
                      "total_tokens": nprompt + ntok},
        }

    async def openai_completions(self, body: Dict[str, Any], model_name: str):
        if body.get("suffix"):
            # fill-in-middle needs a FIM-trained model + template; honest
            # 422 instead of silently generating without the suffix
            raise ValueError(
                "'suffix' (fill-in-middle) is not supported; omit it")
        prompt = body.get("prompt") or ""
        if isinstance(prompt, list):
            prompt = prompt[0] if prompt else ""
        n = self._n_choices(body)
        params = self._choice_params(body, n)
        rid = "cmpl-" + uuid.uuid4().hex[:24]
        lora_idx = self._resolve_lora(body.get("model"))
        if lora_idx >= 0:
            model_name = body["model"]
        if body.get("stream"):
            opts = body.get("stream_options") or {}
            return self._sse_stream(prompt, params[0], rid, model_name,
                                    chat=False,
                                    include_usage=bool(
                                        opts.get("include_usage")),
                                    lora_idx=lora_idx)
        results = await asyncio.gather(
            *[self._collect(prompt, p, lora_idx) for p in params])
        nprompt = results[0][3]
        ntok = sum(r[2] for r in results)
        echo = bool(body.get("echo"))
        prompt_lps: List[dict] = []
        if echo and params[0].logprobs is not None:
            ids = self.tokenizer.encode(prompt)
            if len(ids) > 1:
                prompt_lps = await asyncio.to_thread(
                    self._prompt_logprobs_sync, ids, params[0].logprobs,
                    lora_idx)
            if ids:
                # the first prompt token has no predecessor: null logprob
                prompt_lps = [{"token_ids": [ids[0]], "logprob": None,
                               "top_logprobs": {}}] + prompt_lps
        choices = []
        for i, r in enumerate(results):
            choice = {"index": i,
                      "text": (prompt + r[0]) if echo else r[0],
                      "finish_reason": r[1]}
            if params[i].logprobs is not None:
                choice["logprobs"] = self._completion_logprobs(
                    prompt_lps + r[4])
            choices.append(choice)
        return {
            "id": rid, "object": "text_completion", "created": int(time.time()),
            "model": model_name,
            "choices": choices,
            "usage": {"prompt_tokens": nprompt, "completion_tokens": ntok,
                      "total_tokens": nprompt + ntok},
        }

    def openai_models(self, model_name: str):
        data = [{"id": model_name, "object": "model",
                 "owned_by": "clearml-serving-amd"}]
        if self.lora_bank is not None:
            # adapters are addressable ids of their own (vLLM's layout:
            # parent = the base model, root = where the adapter came from)
            for name, path in zip(self.lora_bank.names,
                                  self.lora_bank.paths):
                data.append({"id": name, "object": "model",
                             "owned_by": "clearml-serving-amd",
                             "parent": model_name, "root": path})
        return {"object": "list", "data": data}

    async def openai_embeddings(self, body: Dict[str, Any], model_name: str):
        inp = body.get("input")
        if inp is None:
            raise ValueError("embeddings request requires 'input'")
        texts = inp if isinstance(inp, list) else [inp]
        vecs = await self.embed_batch([str(t) for t in texts])
        nprompt = sum(len(self.tokenizer.encode(str(t))) for t in texts)
        return {
            "object": "list", "model": model_name,
            "data": [{"object": "embedding", "index": i, "embedding": v}
                     for i, v in enumerate(vecs)],
            "usage": {"prompt_tokens": nprompt, "total_tokens": nprompt},
        }

    async def openai_pooling(self, body: Dict[str, Any], model_name: str):
        """vLLM-style /pooling: raw mean-pooled hidden states (no L2
        normalization, unlike /v1/embeddings)."""
        inp = body.get("input")
        if inp is None:
            raise ValueError("pooling request requires 'input'")
        texts = inp if isinstance(inp, list) else [inp]
        prompts = [self.tokenizer.encode(str(t))[:self.cfg.max_model_len]
                   for t in texts]
        plan = {"mode": "embed", "prompts": prompts, "normalize": False}
        out = await asyncio.to_thread(self._embed_sync, plan)
        return {"object": "list", "model": model_name,
                "data": [{"object": "pooling", "index": i, "data": v}
                         for i, v in enumerate(out)]}

    async def openai_score(self, body: Dict[str, Any], model_name: str):
        """Bi-encoder similarity score between text_1 and text_2 (cosine of
        pooled embeddings). The reference delegates to vLLM cross-encoder
        models (preprocess_service.py:632-1095); with a decoder-only model
        the bi-encoder cosine is the native equivalent."""
        t1 = body.get("text_1")
        t2 = body.get("text_2")
        if t1 is None or t2 is None:
            raise ValueError("score request requires 'text_1' and 'text_2'")
        rights = t2 if isinstance(t2, list) else [t2]
        vecs = await self.embed_batch([str(t1)] + [str(r) for r in rights])
        q = vecs[0]
        scores = [sum(a * b for a, b in zip(q, v)) for v in vecs[1:]]
        return {"object": "list", "model": model_name,
                "data": [{"object": "score", "index": i, "score": s}
                         for i, s in enumerate(scores)]}

    async def openai_rerank(self, body: Dict[str, Any], model_name: str):
        query = body.get("query")
        docs = body.get("documents") or []
        if query is None or not docs:
            raise ValueError("rerank request requires 'query' and 'documents'")
        vecs = await self.embed_batch([str(query)] + [str(d) for d in docs])
        q = vecs[0]
        scored = sorted(
            ((sum(a * b for a, b in zip(q, v)), i)
             for i, v in enumerate(vecs[1:])), reverse=True)
        top_n = body.get("top_n") or len(docs)
        return {"model": model_name, "results": [
            {"index": i, "document": {"text": str(docs[i])},
             "relevance_score": s} for s, i in scored[:top_n]]}

    def openai_tokenize(self, body: Dict[str, Any]):
        prompt = body.get("prompt")
        if prompt is None and body.get("messages"):
            prompt = self._chat_prompt(body["messages"])
        ids = self.tokenizer.encode(prompt or "")
        return {"tokens": ids, "count": len(ids),
                "max_model_len": self.cfg.max_model_len}

    def openai_detokenize(self, body: Dict[str, Any]):
        return {"prompt": self.tokenizer.decode(body.get("tokens") or [])}

    async def _collect(self, prompt: str, params: SamplingParams,
                       lora_idx: int = -1):
        ids = self.tokenizer.encode(prompt)
        tokens: List[int] = []
        reason = None
        lps: List[dict] = []
        async for item in self.generate(prompt, params, lora_idx):
            if item.get("error"):
                # engine-side failure: surface it (the route maps to 500)
                # instead of returning truncated text as if successful
                raise RuntimeError("generation failed: {}".format(
                    item["error"]))
            tokens.extend(item.get("token_ids", []))
            if "logprob" in item:
                lps.append({"token_ids": item["token_ids"],
                            "logprob": item["logprob"],
                            "top_logprobs": item.get("top_logprobs") or {}})
            reason = item.get("finish_reason") or reason
        text = self._truncate_at_stop(
            self.tokenizer.decode(tokens), params, reason)
        return text, reason, len(tokens), len(ids), lps

    def _prompt_logprobs_sync(self, ids: List[int], k: int,
                              lora_idx: int = -1) -> List[dict]:
        """Teacher-forced logprobs of the prompt tokens themselves (the
        completions echo+logprobs contract): row i-1's distribution scores
        token i; the first token has no predecessor (None upstream).
        Runs under the exec lock like the embed path."""
        with self._exec_lock:
            with torch.inference_mode():
                dev = self.device
                n = len(ids)
                tokens = torch.tensor(ids, dtype=torch.long, device=dev)
                positions = torch.arange(n, dtype=torch.int32, device=dev)
                attn_ctx = {
                    "mode": "prefill", "batch": 1, "seq": n,
                    "seq_lens": torch.tensor([n], dtype=torch.int32,
                                             device=dev),
                    "slot_mapping": torch.full((n,), -1, dtype=torch.int32,
                                               device=dev),
                }
                if lora_idx >= 0:
                    self._lora_ctx(attn_ctx, [lora_idx] * n)
                logits = self.model(tokens, positions, kv_caches=None,
                                    attn_ctx=attn_ctx)
                lsm = torch.log_softmax(logits.float(), dim=-1)
        out = []
        for i in range(1, n):
            row = lsm[i - 1]
            e = {"token_ids": [ids[i]], "logprob": float(row[ids[i]])}
            if k:
                topv, topi = row.topk(k)
                e["top_logprobs"] = {
                    int(t): float(v)
                    for v, t in zip(topv.tolist(), topi.tolist())}
            else:
                e["top_logprobs"] = {}
            out.append(e)
        return out

    def _lp_entry(self, tok_id: int, logprob: float,
                  top: Dict[int, float]) -> dict:
        tokstr = self.tokenizer.decode([tok_id])
        return {"token": tokstr, "logprob": logprob,
                "bytes": list(tokstr.encode()),
                "top_logprobs": [
                    {"token": self.tokenizer.decode([t]), "logprob": v}
                    for t, v in top.items()]}

    def _chat_logprobs(self, lps: List[dict]) -> Optional[dict]:
        if not lps:
            return None
        return {"content": [
            self._lp_entry(e["token_ids"][0], e["logprob"],
                           e["top_logprobs"]) for e in lps]}

    def _completion_logprobs(self, lps: List[dict]) -> Optional[dict]:
        if not lps:
            return None
        tops = []
        for e in lps:
            d: Dict[str, float] = {}
            for t, v in e["top_logprobs"].items():
                # this format keys by decoded STRING; ids that decode to
                # the same text keep the max (never shadow the top-1)
                k = self.tokenizer.decode([t])
                if k not in d or v > d[k]:
                    d[k] = v
            tops.append(d)
        return {
            "tokens": [self.tokenizer.decode(e["token_ids"]) for e in lps],
            "token_logprobs": [e["logprob"] for e in lps],
            "top_logprobs": tops,
            "text_offset": [],
        }

    def _sse_stream(self, prompt: str, params: SamplingParams, rid: str,
                    model_name: str, chat: bool,
                    include_usage: bool = False, lora_idx: int = -1):
        from fastapi.responses import StreamingResponse

        async def gen():
            ntok = 0
            async for item in self.generate(prompt, params, lora_idx):
                ntok += len(item.get("token_ids", []))
                if item.get("error"):
                    yield "data: {}\n\n".format(json.dumps(
                        {"error": {"message": str(item["error"]),
                                   "type": "engine_error"}}))
                    break
                if chat:
                    delta = {"content": item.get("text", "")}
                    choice = {"index": 0, "delta": delta,
                              "finish_reason": item.get("finish_reason")}
                    obj = "chat.completion.chunk"
                else:
                    choice = {"index": 0, "text": item.get("text", ""),
                              "finish_reason": item.get("finish_reason")}
                    obj = "text_completion"
                if "logprob" in item:
                    entry = self._lp_entry(item["token_ids"][0],
                                           item["logprob"],
                                           item.get("top_logprobs") or {})
                    choice["logprobs"] = ({"content": [entry]} if chat
                                          else {"tokens": [entry["token"]],
                                                "token_logprobs":
                                                    [entry["logprob"]]})
                chunk = {"id": rid, "object": obj,
                         "created": int(time.time()), "model": model_name,
                         "choices": [choice]}
                yield "data: {}\n\n".format(json.dumps(chunk))
            if include_usage:
                # OpenAI stream_options.include_usage: one final chunk
                # with empty choices and the usage totals
                nprompt = len(self.tokenizer.encode(prompt))
                yield "data: {}\n\n".format(json.dumps({
                    "id": rid,
                    "object": ("chat.completion.chunk" if chat
                               else "text_completion"),
                    "created": int(time.time()), "model": model_name,
                    "choices": [],
                    "usage": {"prompt_tokens": nprompt,
                              "completion_tokens": ntok,
                              "total_tokens": nprompt + ntok}}))
            yield "data: [DONE]\n\n"

        return StreamingResponse(gen(), media_type="text/event-stream")
