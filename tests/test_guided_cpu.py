"""Guided decoding on the CPU: the regex/schema -> DFA front end, token
masks, the ops CPU references and the engine end to end (llama-tiny, random
weights: every assertion is a property of the grammar, not of the model)."""

import asyncio
import json
import os
import random
import re
import sys

import numpy as np
import pytest
import torch
from hypothesis import given, settings
from hypothesis import strategies as st

from clearml_serving_amd import ops
from clearml_serving_amd.engines.llm import guided as G
from clearml_serving_amd.engines.llm.engine import (
    HfTokenizer, LlmEngine, LlmEngineConfig, SamplingParams, SimpleTokenizer)
from clearml_serving_amd.models.llama import PRESETS

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))
import lora_util  # noqa: E402

# --------------------------------------------------------------------- #
# regex -> DFA
# --------------------------------------------------------------------- #
PATTERNS = {
    r"[0-9]{3}-[a-f]{2}": ["123-ab", "12-ab", "123-ag", "1234-ab", ""],
    r"(ab|cd)*e?": ["", "e", "abcd", "abce", "abc", "ee"],
    r"[^abc]+x": ["dx", "ax", "x", "ééx", "d\nx"],
    r"\d+\.\d{1,3}": ["1.5", "12.345", "1.2345", ".5", "1."],
    r"a{2,}b{0,2}": ["aa", "a", "aaabb", "aabbb"],
    r"(a|(bc|d){2})+": ["a", "bcd", "dd", "abcbca", "bc", "d"],
    r"é+z|日本": ["éz", "ééz", "z", "日本", "日"],
    r".*": ["", "anything é", "a\nb"],
    r"[\w.-]+@[a-z]+\.(com|org)": ["a.b-c@foo.com", "a@b.net", "@b.com"],
    r"[]a]+|[b\]]": ["]a", "b", "]", "ab"],
    r"\S\s[^\d\s]": ["a b", "é\té", "a 1", "  a"],
    r"x{2}y{,3}|\x41é\t": ["xx", "xxy{,3}", "Aé\t", "xxyyy"],
    r"(?:no|yes)+?!*?": ["no", "yesno!!", "!", ""],
}
ALPHABET = "ab cdexyz019.-@]\n\té日本A!{},"


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_dfa_agrees_with_re_on_picked_strings(pattern):
    dfa = G.compile_regex(pattern)
    for s in PATTERNS[pattern]:
        want = re.fullmatch(pattern, s, re.ASCII) is not None
        assert dfa.matches(s) == want, (pattern, s)


_DFAS = {p: G.compile_regex(p) for p in PATTERNS}


@settings(max_examples=300, deadline=None)
@given(st.sampled_from(sorted(PATTERNS)),
       st.text(alphabet=ALPHABET, max_size=8))
def test_dfa_agrees_with_re_on_generated_strings(pattern, s):
    want = re.fullmatch(pattern, s, re.ASCII) is not None
    assert _DFAS[pattern].matches(s) == want, (pattern, s)


@pytest.mark.parametrize("pattern,construct", [
    (r"(a)\1", "backreference"), (r"a(?=b)", "lookaround"),
    (r"(?<!a)b", "lookaround"), (r"^ab", "anchor"), (r"ab$", "anchor"),
    (r"a\b", "boundary"), (r"(?P<n>a)", "named"), (r"(?i)a", "flags"),
    (r"a*+", "possessive"), (r"[^é]", "negated class"),
    (r"[а-я]", "range"), (r"\pL", "escape"),
])
def test_unsupported_regex_constructs_name_themselves(pattern, construct):
    with pytest.raises(ValueError, match=construct):
        G.compile_regex(pattern)


def test_malformed_regex_and_empty_language_raise():
    for bad in ("(ab", "ab)", "[ab", "*a", "a{3,2}", "a\\"):
        with pytest.raises(ValueError):
            G.compile_regex(bad)
    with pytest.raises(ValueError, match="matches no string"):
        G.compile_ast(("set", 0))


def test_state_cap_raises_too_complex():
    with pytest.raises(ValueError, match="too complex"):
        G.compile_regex("(a|b)*a(a|b){12}", max_states=500)
    assert G.compile_regex("(a|b)*a(a|b){3}", max_states=500).n_states <= 32


def test_dead_states_are_pruned():
    dfa = G.compile_regex("ab|ac")
    # start, "a", "ab", "ac" (no minimisation); the sink is the extra row
    assert dfa.n_states == 4 and dfa.step(0, b"ad") == dfa.dead
    assert (dfa.trans[dfa.dead] == dfa.dead).all()


# --------------------------------------------------------------------- #
# JSON schema
# --------------------------------------------------------------------- #
def check(value, schema, root=None):
    """Minimal validator for the supported schema subset."""
    root = schema if root is None else root
    if "$ref" in schema:
        node = root
        for part in schema["$ref"][2:].split("/"):
            node = node[part]
        return check(value, node, root)
    if "const" in schema:
        return value == schema["const"] and type(value) is type(
            schema["const"])
    if "enum" in schema:
        return any(value == e and type(value) is type(e)
                   for e in schema["enum"])
    if "anyOf" in schema:
        return any(check(value, s, root) for s in schema["anyOf"])
    t = schema.get("type")
    if isinstance(t, list):
        return any(check(value, {**schema, "type": one}, root) for one in t)
    if t == "object":
        props = schema.get("properties", {})
        return (isinstance(value, dict)
                and all(k in value for k in schema.get("required", []))
                and all(k in props and check(v, props[k], root)
                        for k, v in value.items())
                and list(value) == [k for k in props if k in value])
    if t == "array":
        return (isinstance(value, list)
                and schema.get("minItems", 0) <= len(value)
                <= schema.get("maxItems", 10**9)
                and all(check(v, schema.get("items", {}), root)
                        for v in value))
    if t == "string":
        return (isinstance(value, str)
                and schema.get("minLength", 0) <= len(value)
                <= schema.get("maxLength", 10**9)
                and ("pattern" not in schema or re.fullmatch(
                    schema["pattern"], value, re.ASCII) is not None))
    if t == "integer":
        return isinstance(value, int) and not isinstance(value, bool)
    if t == "number":
        return isinstance(value, (int, float)) and not isinstance(value, bool)
    if t == "boolean":
        return isinstance(value, bool)
    if t == "null":
        return value is None
    return t is None


def random_walk(dfa, rng, max_len=400):
    """A random accepted byte string: follow live transitions, stopping at
    accepting states with rising probability."""
    state, out = 0, bytearray()
    while True:
        nxt = np.nonzero(dfa.trans[state] != dfa.dead)[0]
        if dfa.accept[state] and (len(nxt) == 0 or rng.random() < 0.15
                                  or len(out) > max_len):
            return bytes(out)
        if len(out) > max_len:  # head for an exit: ascii closers first
            pref = [b for b in nxt if chr(b) in '"}]' or chr(b).isalnum()]
            nxt = pref or nxt
        b = int(rng.choice(list(nxt)))
        out.append(b)
        state = int(dfa.trans[state, b])


BIG_SCHEMA = {
    "$defs": {"tag": {"type": "string", "minLength": 1, "maxLength": 4},
              "point": {"type": "object", "required": ["x"],
                        "properties": {"x": {"type": "number"},
                                       "y": {"type": ["integer", "null"]}}}},
    "type": "object",
    "required": ["kind", "id", "pos"],
    "properties": {
        "kind": {"enum": ["circle", "square", 3, None]},
        "id": {"type": "string", "pattern": "[A-Z]{2}-\\d{1,4}"},
        "ok": {"type": "boolean"},
        "pos": {"$ref": "#/$defs/point"},
        "tags": {"type": "array", "items": {"$ref": "#/$defs/tag"},
                 "minItems": 1, "maxItems": 3},
        "version": {"const": "v1"},
        "extra": {"anyOf": [{"type": "null"},
                            {"type": "array", "items": {"type": "integer"}},
                            {"type": "string", "maxLength": 2}]},
        "pairs": {"type": "array", "minItems": 2,
                  "items": {"type": "boolean"}},
    },
}
SCHEMAS = {
    "big": BIG_SCHEMA,
    "string": {"type": "string", "minLength": 2, "maxLength": 6},
    "integer": {"type": "integer"},
    "number": {"type": "number"},
    "array": {"type": "array", "items": {"type": "integer"},
              "minItems": 2, "maxItems": 4},
    "array_open": {"type": "array", "items": {"type": "null"},
                   "minItems": 3},
    "all_optional": {"type": "object", "properties": {
        "a": {"type": "boolean"}, "b": {"type": "null"},
        "c": {"type": "integer"}}},
    "top_enum": {"enum": ["a b", 1, True, {"k": [1, 2]}]},
    "top_anyof": {"anyOf": [{"type": "boolean"}, {"const": "é\"q"}]},
}


@pytest.mark.parametrize("name", sorted(SCHEMAS))
def test_schema_dfa_generates_only_valid_documents(name):
    schema = SCHEMAS[name]
    dfa = G.compile_ast(G.schema_ast(schema))
    rng = random.Random(7)
    seen = set()
    for _ in range(60):
        text = random_walk(dfa, rng).decode("utf-8")
        seen.add(text)
        assert check(json.loads(text), schema), text
    assert len(seen) > 1


def test_schema_rejects_invalid_documents():
    dfa = G.compile_ast(G.schema_ast(BIG_SCHEMA))
    good = '{"kind":"circle", "id":"AB-12","pos":{"x":1.5e3,"y":null}}'
    assert dfa.matches(good)
    assert dfa.matches('{"kind":3,"id":"AB-1","ok":true,"pos":{"x":0},'
                       '"tags":["a","bcde"],"pairs":[true, false,true]}')
    for bad in [
        '{"id":"AB-12","pos":{"x":1}}',                      # kind missing
        '{"kind":"circle","id":"ab-12","pos":{"x":1}}',      # pattern
        '{"kind":"circle","id":"AB-12","pos":{"y":1}}',      # nested required
        '{"kind":"circle","id":"AB-12","pos":{"x":1},"tags":[]}',  # minItems
        '{"kind":"circle","id":"AB-12","pos":{"x":1},'
        '"tags":["a","b","c","d"]}',                         # maxItems
        '{"kind":"circle","id":"AB-12","pos":{"x":1},"tags":["abcde"]}',
        '{"kind":"circle","id":"AB-12","pos":{"x":1},"zzz":1}',  # additional
        '{"id":"AB-12","kind":"circle","pos":{"x":1}}',      # declared order
        '{"kind":"circle","id":"AB-12","pos":{"x":1},"pairs":[true]}',
        '{"kind":"circle","id":"AB-12","pos":{"x":1},"version":"v2"}',
        '{"kind": "circle" ,"id":"AB-12","pos":{"x":1}}',    # whitespace
        '{"kind":"circle","id":"AB-12","pos":{"x":01}}',     # leading zero
        '{"kind":"circle","id":"AB-12","pos":{"x":1},}',
    ]:
        assert not dfa.matches(bad), bad


@pytest.mark.parametrize("schema,word", [
    ({"$defs": {"n": {"type": "object", "properties": {
        "next": {"$ref": "#/$defs/n"}}}}, "$ref": "#/$defs/n"}, "recursive"),
    ({"oneOf": [{"type": "null"}]}, "oneOf"),
    ({"allOf": [{"type": "null"}]}, "allOf"),
    ({"not": {"type": "null"}}, "not"),
    ({"type": "object", "patternProperties": {"a": {}}}, "patternProperties"),
    ({"if": {"type": "null"}}, "if"),
    ({"type": "integer", "minimum": 3}, "minimum"),
    ({"$ref": "http://x/y"}, "ref"),
    ({"type": "frob"}, "type"),
])
def test_unsupported_schema_raises(schema, word):
    with pytest.raises(ValueError, match=word):
        G.schema_ast(schema)


def nested(depth):
    doc = "1"
    for i in range(depth):
        doc = '{"k":%s}' % doc if i % 2 == 0 else "[%s]" % doc
    return doc if depth % 2 else '{"k":%s}' % doc


def test_json_object_depth_bound():
    dfa = G.compile_ast(G.json_object_ast(4))
    assert dfa.matches("{}") and not dfa.matches("[]")
    assert dfa.matches('{"a":"x\\n\\u00e9é","b":-1.5e3,"c":null, "d":[]}')
    deep4 = '{"a":{"b":[1,{"c":true}]}}'
    deep5 = '{"a":{"b":[1,{"c":[]}]}}'
    assert dfa.matches(deep4) and not dfa.matches(deep5)
    assert G.compile_ast(G.json_object_ast(5)).matches(deep5)
    rng = random.Random(3)
    for _ in range(30):
        assert isinstance(json.loads(random_walk(dfa, rng)), dict)


# --------------------------------------------------------------------- #
# vocabulary + masks
# --------------------------------------------------------------------- #
def bytelevel_tokenizer(tmp_path):
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers
    from tokenizers import trainers

    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    trainer = trainers.BpeTrainer(
        vocab_size=400, special_tokens=["<|endoftext|>", "<|pad|>"],
        initial_alphabet=pre_tokenizers.ByteLevel.alphabet())
    corpus = ['{"kind": "circle", "id": "AB-12", "ok": true}',
              "the quick brown fox 123-ab 456-cd née 日本",
              '[1, 2, 3] {"a": null, "b": false}'] * 8
    tok.train_from_iterator(corpus, trainer)
    path = str(tmp_path / "tokenizer.json")
    tok.save(path)
    return HfTokenizer(path)


def naive_mask(vocab, dfa, state):
    out = np.zeros(vocab.words * 32, dtype=bool)
    for tid, data in enumerate(vocab.token_bytes):
        if data and dfa.step(state, data) != dfa.dead:
            out[tid] = True
    return out


def reachable_states(dfa, n, rng):
    states, state = [0], 0
    for _ in range(200):
        nxt = np.nonzero(dfa.trans[state] != dfa.dead)[0]
        if len(nxt) == 0:
            state = 0
            continue
        state = int(dfa.trans[state, rng.choice(list(nxt))])
        if state not in states:
            states.append(state)
    return states[:n]


@pytest.mark.parametrize("kind", ["simple", "bpe"])
def test_vectorised_mask_equals_naive_walk(kind, tmp_path):
    tok = SimpleTokenizer() if kind == "simple" \
        else bytelevel_tokenizer(tmp_path)
    width = tok.vocab_size + 70  # model vocab padded past the tokenizer
    comp = G.GuidedCompiler(tok, width)
    vocab = comp.vocab
    assert vocab.token_bytes[tok.eos_id] is None
    if kind == "bpe":
        # ByteLevel: every single byte is a token, merges are longer ones
        assert {b for b in vocab.token_bytes if b and len(b) == 1} == {
            bytes([i]) for i in range(256)}
        assert max(len(b) for b in vocab.token_bytes if b) > 1
        assert vocab.token_bytes[tok._tok.token_to_id("<|pad|>")] is None
        text = "née 日本 123-ab"
        assert b"".join(vocab.token_bytes[i] for i in tok.encode(text)) \
            == text.encode("utf-8")
    grammar = comp.compile("json", BIG_SCHEMA)
    assert comp.compile("json", json.dumps(BIG_SCHEMA)) is grammar  # LRU
    dfa = grammar.dfa
    rng = random.Random(1)
    for state in reachable_states(dfa, 12, rng):
        gs = G.GuidedState(grammar, [tok.eos_id])
        gs.state = state
        want = naive_mask(vocab, dfa, state)
        allowed, count = grammar.token_mask(state)
        assert (allowed == want).all() and count == want.sum()
        words = gs.mask_words()
        assert words.dtype == np.int32 and words.shape == (vocab.words,)
        bits = (words.view(np.uint32)[:, None] >> np.arange(32)) & 1
        bits = bits.reshape(-1).astype(bool)
        want[tok.eos_id] = gs.accepting()
        assert (bits == want).all()
        assert not bits[tok.vocab_size:].any()   # ids past the tokenizer
        assert not bits[width:].any()            # bits >= V
    # eos / stop ids follow acceptance; a stop id that is also a byte token
    # is allowed ONLY as a finish
    g2 = comp.compile("regex", "ab?")
    stop = tok.encode("b")[0]
    gs = G.GuidedState(g2, [tok.eos_id, stop])
    assert not gs.allows(tok.eos_id) and not gs.allows(stop)
    gs.advance(tok.encode("a")[0])
    assert gs.accepting() and gs.allows(tok.eos_id) and gs.allows(stop)
    assert gs.num_continuations() == 0  # "b" only finishes now
    plain = G.GuidedState(g2, [tok.eos_id])
    plain.advance(tok.encode("a")[0])
    assert plain.num_continuations() == 1
    plain.advance(tok.encode("b")[0])
    assert plain.accepting() and plain.num_continuations() == 0


def test_non_byte_tokenizer_makes_engine_start_raise(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "examples", "llm"))
    import make_tiny_checkpoint

    path = make_tiny_checkpoint.train_tokenizer(str(tmp_path))
    cfg = LlmEngineConfig(preset="llama-tiny", num_kv_blocks=16,
                          max_model_len=64, device="cpu",
                          tokenizer_path=path, guided_decoding=True)
    with pytest.raises(ValueError, match="byte-level"):
        LlmEngine(cfg).start()
    cfg.guided_decoding = False
    LlmEngine(cfg).start()  # same tokenizer serves unguided


def test_config_validation_and_from_aux(tmp_path):
    with pytest.raises(ValueError, match="guided_mask_slots"):
        LlmEngine(LlmEngineConfig(
            preset="llama-tiny", num_kv_blocks=16, device="cpu",
            guided_decoding=True, guided_mask_slots=8,
            max_num_seqs=16)).start()
    card = tmp_path / "card.json"
    card.write_text(json.dumps({"preset": "llama-tiny",
                                "guided_decoding": True,
                                "guided_json_depth": 2}))
    cfg = LlmEngineConfig.from_aux(str(card), {"guided_mask_slots": 99,
                                               "guided_max_states": 123})
    assert (cfg.guided_decoding, cfg.guided_json_depth,
            cfg.guided_mask_slots, cfg.guided_max_states) == (True, 2, 99,
                                                              123)
    assert LlmEngineConfig().guided_decoding is False


# --------------------------------------------------------------------- #
# ops CPU references
# --------------------------------------------------------------------- #
def pack(allowed):
    rows, vocab = allowed.shape
    words = (vocab + 31) // 32
    padded = np.zeros((rows, words * 32), dtype=bool)
    padded[:, :vocab] = allowed.numpy()
    return torch.from_numpy(np.stack([G.pack_bits(r) for r in padded]))


def test_ops_cpu_references():
    vocab = 70
    allowed = torch.zeros(3, vocab, dtype=torch.bool)
    allowed[0, [1, 33, 69]] = True
    allowed[1] = True
    bank = pack(allowed)
    assert bank.dtype == torch.int32 and bank.shape == (3, 3)
    logits = torch.arange(4 * vocab, dtype=torch.float32).view(4, vocab)
    logits[0, 33] = logits[0, 69] = 500.0  # tie: lowest index wins
    keep = logits.clone()
    slot = torch.tensor([0, -1, 1, 2], dtype=torch.int32)
    out = ops.apply_token_bitmask(logits, bank, slot)
    assert torch.equal(logits, keep)
    assert torch.equal(out[1], logits[1]) and torch.equal(out[2], logits[2])
    assert torch.isinf(out[3]).all() and (out[3] < 0).all()
    assert torch.equal(out[0, [1, 33, 69]], logits[0, [1, 33, 69]])
    assert torch.isinf(out[0]).sum() == vocab - 3
    zeros = torch.zeros(4)
    seed = torch.zeros(4, dtype=torch.int32)
    got = ops.sample_token_bitmask(logits, bank, slot, zeros, seed)
    assert got.tolist() == [33, vocab - 1, vocab - 1, -1]
    for s in range(20):
        got = ops.sample_token_bitmask(
            logits * 0, bank, slot, torch.ones(4),
            torch.full((4,), s, dtype=torch.int32))
        assert int(got[0]) in (1, 33, 69) and int(got[3]) == -1
    with pytest.raises(ValueError):
        ops.apply_token_bitmask(logits, bank.long(), slot)
    with pytest.raises(ValueError):
        ops.apply_token_bitmask(logits, bank, slot.long())
    with pytest.raises(ValueError):
        ops.apply_token_bitmask(logits, bank[:, :2], slot)


# --------------------------------------------------------------------- #
# engine
# --------------------------------------------------------------------- #
REGEX = "[0-9]{3}-[a-f]{2}"
CHOICES = ["alpha", "beta", "alphabet"]
BOUNDED = {"type": "object", "required": ["kind", "n"], "properties": {
    "kind": {"enum": ["cat", "dog"]}, "ok": {"type": "boolean"},
    "n": {"type": "string", "pattern": "[0-9]{1,4}"},
    "s": {"type": "string", "maxLength": 5},
    "xs": {"type": "array", "maxItems": 2, "items": {"type": "boolean"}}}}


def make_engine(**kw):
    cfg = dict(preset="llama-tiny", num_kv_blocks=64, block_size=16,
               max_model_len=256, device="cpu", guided_decoding=True)
    cfg.update(kw)
    eng = LlmEngine(LlmEngineConfig(**cfg))
    eng.start()
    return eng


@pytest.fixture(scope="module")
def eng():
    return make_engine()


def generate(eng, bodies, prompts=None, lora=None):
    """All requests in flight together -> [(text, reason, ids, items)]."""
    prompts = prompts or ["prompt {}".format(i) for i in range(len(bodies))]

    async def one(i):
        params = SamplingParams.from_request(
            {"max_tokens": 120, **bodies[i]},
            guided=eng.cfg.guided_decoding)
        ids, items, reason = [], [], None
        async for item in eng.generate(prompts[i], params,
                                       lora[i] if lora else -1):
            assert not item.get("error"), item
            ids.extend(item["token_ids"])
            items.append(item)
            reason = item.get("finish_reason") or reason
        return eng.tokenizer.decode(ids), reason, ids, items

    async def main():
        return await asyncio.gather(*[one(i) for i in range(len(bodies))])

    return lora_util.run(main())


@pytest.mark.parametrize("sampling", [
    {"temperature": 0.0}, {"temperature": 1.0, "seed": 4}],
    ids=["greedy", "seeded"])
def test_engine_outputs_match_their_grammar(eng, sampling):
    outs = generate(eng, [
        {"guided_regex": REGEX, **sampling},
        {"guided_choice": CHOICES, **sampling},
        {"guided_json": BOUNDED, **sampling},
        {"structured_outputs": {"regex": REGEX}, **sampling},
        {"response_format": {"type": "json_schema", "json_schema": {
            "name": "x", "schema": BOUNDED}}, **sampling},
        {"guided_json": json.dumps(BOUNDED), **sampling},
    ])
    assert all(o[1] == "stop" for o in outs), [(o[0], o[1]) for o in outs]
    assert re.fullmatch(REGEX, outs[0][0]) and re.fullmatch(REGEX, outs[3][0])
    assert outs[1][0] in CHOICES
    for o in (outs[2], outs[4], outs[5]):
        assert check(json.loads(o[0]), BOUNDED), o[0]
    if "seed" in sampling:  # per-request reproducibility
        again = generate(eng, [{"guided_json": BOUNDED, **sampling}],
                         prompts=["prompt 2"])
        assert again[0][2] == outs[2][2]


def test_json_object_mode_parses_when_it_stops(eng):
    outs = generate(eng, [{"response_format": {"type": "json_object"},
                           "temperature": 1.0, "seed": s, "max_tokens": 60}
                          for s in range(4)])
    for text, reason, ids, _ in outs:
        if reason == "stop":
            assert isinstance(json.loads(text), dict)
        else:  # ran out of tokens: still a prefix of some JSON object
            assert reason == "length" and text.startswith("{")


def test_mixed_batch_leaves_unguided_requests_alone(eng):
    free = {"temperature": 0.0, "ignore_eos": True, "max_tokens": 10}
    pen = {**free, "repetition_penalty": 1.3}
    alone = generate(eng, [free], prompts=["the free one"])
    alone_pen = generate(eng, [pen], prompts=["the free one"])
    mixed = generate(eng, [
        {"guided_regex": REGEX, "temperature": 0.0}, free,
        {"guided_json": BOUNDED, "temperature": 1.0, "seed": 2}, pen],
        prompts=["a", "the free one", "b", "the free one"])
    assert mixed[1][2] == alone[0][2] and len(alone[0][2]) == 10
    assert mixed[3][2] == alone_pen[0][2]
    assert re.fullmatch(REGEX, mixed[0][0])
    assert check(json.loads(mixed[2][0]), BOUNDED)


def test_logprobs_are_of_the_masked_distribution(eng):
    grammar = eng.guided_compiler.compile("regex", REGEX)
    out = generate(eng, [{"guided_regex": REGEX, "temperature": 0.0,
                          "logprobs": 5}])[0]
    assert re.fullmatch(REGEX, out[0])
    state = G.GuidedState(grammar, [eng.tokenizer.eos_id])
    for item in out[3]:
        tok = item["token_ids"][0]
        finite = {t: v for t, v in item["top_logprobs"].items()
                  if v > float("-inf")}
        assert finite and all(state.allows(t) for t in finite)
        assert state.allows(tok) and item["logprob"] <= 0.0
        state.advance(tok)


def test_penalties_n_and_streaming(eng):
    out = generate(eng, [{"guided_regex": "[ab]{6}", "temperature": 0.0,
                          "repetition_penalty": 1.5,
                          "presence_penalty": 0.5, "top_k": 4}])[0]
    assert re.fullmatch("[ab]{6}", out[0]) and out[1] == "stop"
    assert "".join(i["text"] for i in out[3]) == out[0]  # stream deltas

    async def n2():
        return await eng.openai_completions(
            {"prompt": "x", "n": 2, "seed": 9, "temperature": 1.0,
             "max_tokens": 40, "guided_choice": CHOICES}, "m")

    resp = lora_util.run(n2())
    assert len(resp["choices"]) == 2
    assert all(c["text"] in CHOICES and c["finish_reason"] == "stop"
               for c in resp["choices"])


def test_lora_adapter_with_guided_request(tmp_path):
    mcfg = PRESETS["llama-tiny"]
    lora_util.write_adapter(str(tmp_path / "a"), mcfg, lora_util.ALL_LINEAR,
                            seed=1, std=0.3)
    eng = make_engine(lora_modules=[{"name": "a",
                                     "path": str(tmp_path / "a")}])
    body = {"guided_regex": "[a-z]{12}", "temperature": 0.0}
    outs = generate(eng, [body, body], prompts=["same", "same"],
                    lora=[-1, 0])
    assert all(re.fullmatch("[a-z]{12}", o[0]) for o in outs)
    assert outs[0][2] != outs[1][2]  # the adapter still steers the text
    assert eng.stats["lora_requests"] == 1


def test_dfa_state_survives_preemption():
    eng = make_engine(num_kv_blocks=8, block_size=4, max_model_len=64)
    bodies = [{"guided_regex": "[a-z]{24}", "temperature": 0.0}] * 3
    outs = generate(eng, bodies, prompts=["aa", "bb", "cc"])
    assert eng.stats["preemptions"] > 0
    assert all(re.fullmatch("[a-z]{24}", o[0]) and o[1] == "stop"
               for o in outs), [o[0] for o in outs]


def test_prefix_caching_and_chunked_prefill_with_guided():
    eng = make_engine(enable_prefix_caching=True, prefill_chunk=8)
    prompt = "a long shared prompt " * 3
    for _ in range(2):
        out = generate(eng, [{"guided_regex": REGEX, "temperature": 0.0}],
                       prompts=[prompt])[0]
        assert re.fullmatch(REGEX, out[0])
    assert eng.stats.get("prefix_cache_hit_tokens", 0) > 0


def test_speculative_engine_serves_guided_by_plain_decode():
    eng = make_engine(speculative={"method": "ngram", "num_spec_tokens": 3})
    out = generate(eng, [{"guided_regex": "(ab){8}", "temperature": 0.0}],
                   prompts=["abababab"])[0]
    assert out[0] == "ab" * 8 and eng.stats["spec_proposed"] == 0


def test_refused_combinations(eng):
    for extra in ({"ignore_eos": True}, {"min_tokens": 2},
                  {"guided_choice": ["a"]},
                  {"response_format": {"type": "json_object"}},
                  {"structured_outputs": {"json": {}}}):
        with pytest.raises(ValueError):
            SamplingParams.from_request({"guided_regex": "a+", **extra},
                                        guided=True)
    for body in ({"guided_regex": "(a"}, {"guided_regex": ""},
                 {"guided_choice": []}, {"guided_choice": "ab"},
                 {"guided_json": "{not json"}, {"guided_json": 3},
                 {"structured_outputs": {"grammar": "x"}},
                 {"response_format": {"type": "json_schema"}},
                 {"response_format": {"type": "xml"}}):
        with pytest.raises(ValueError):
            p = SamplingParams.from_request(body, guided=True)
            eng._guided_state(p)
    with pytest.raises(ValueError, match="oneOf"):
        eng._guided_state(SamplingParams.from_request(
            {"guided_json": {"oneOf": []}}, guided=True))
    # a constraint smuggled past from_request still cannot ignore eos
    with pytest.raises(ValueError):
        eng._guided_state(SamplingParams(guided=("regex", "a+"),
                                         ignore_eos=True))
    # tensor parallelism: refused at start
    tp = LlmEngine(LlmEngineConfig(preset="llama-tiny", device="cpu",
                                   guided_decoding=True))
    tp.tp_size, tp.cfg.guided_mask_slots = 2, 1024
    with pytest.raises(ValueError, match="tensor parallelism"):
        tp._start_guided(PRESETS["llama-tiny"])


def test_guided_fields_refused_when_the_engine_has_it_off():
    with pytest.raises(ValueError, match="guided_decoding"):
        SamplingParams.from_request({"guided_regex": "a+"})
    with pytest.raises(ValueError, match="guided_decoding"):
        SamplingParams.from_request({"structured_outputs": {"regex": "a"}})
    with pytest.raises(ValueError, match="no guided-decoding backend"):
        SamplingParams.from_request(
            {"response_format": {"type": "json_object"}})
    off = make_engine(guided_decoding=False)
    assert off.mask_bank is None and "guided_requests" not in off.stats
    with pytest.raises(ValueError, match="guided_decoding"):
        lora_util.run(off.openai_completions(
            {"prompt": "x", "guided_choice": ["a"]}, "m"))
    with pytest.raises(ValueError, match="does not enable"):
        lora_util.run(off.add_request([1, 2], SamplingParams(
            guided=("regex", "a+"))))


def test_dead_end_grammar_finishes_and_counts(eng):
    # ids 1..256 spell every byte, so starve the vocabulary: a model whose
    # logits stop at id 100 cannot spell 'z' (id 123)
    small = make_engine(overrides={"vocab_size": 100})
    before = small.stats["guided_dead_ends"]
    outs = generate(small, [{"guided_regex": "ABz+", "temperature": 0.0},
                            {"guided_regex": "z", "temperature": 0.0}],
                    prompts=["AB 12", "BA 21"])  # ids below 100 only
    assert outs[0][0] == "AB" and outs[0][1] == "stop"
    assert outs[1][2] == [] and outs[1][1] == "stop"
    assert small.stats["guided_dead_ends"] == before + 2


def test_mask_bank_lru_never_evicts_the_current_step():
    stats = {"guided_mask_hits": 0, "guided_mask_misses": 0}
    bank = G.MaskBank(3, 2, torch.device("cpu"), stats)

    def words(v):
        return lambda: np.full(2, v, dtype=np.int32)

    bank.begin_step()
    slots = [bank.acquire(("g", i), words(i)) for i in range(3)]
    assert sorted(slots) == [0, 1, 2] and stats["guided_mask_misses"] == 3
    bank.begin_step()
    assert bank.acquire(("g", 2), words(2)) == slots[2]   # hit
    new = bank.acquire(("g", 9), words(9))                # evicts LRU: 0
    assert new == slots[0] and stats["guided_mask_hits"] == 1
    assert bank.bank[new].tolist() == [9, 9]
    assert bank.acquire(("g", 8), words(8)) == slots[1]
    with pytest.raises(RuntimeError):                     # all 3 in use
        bank.acquire(("g", 7), words(7))
