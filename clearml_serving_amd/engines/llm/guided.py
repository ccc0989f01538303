"""Guided decoding front end: regex / JSON schema / choice -> byte-level DFA
-> per-state token bitmasks (kernels: ops/csrc/token_mask.hip).

No grammar library is needed: a constraint is lowered to a small regex AST,
compiled (Thompson NFA -> subset construction over byte equivalence classes)
to a DFA over UTF-8 BYTES, and the tokenizer's vocabulary is walked through
that DFA to get, per DFA state, the set of tokens that keep the output a
prefix of some accepted string.

Supported regex subset (anchored full match, like ``re.fullmatch``):
literals and escapes (``\\n \\t \\r \\f \\v \\0 \\xHH \\uHHHH`` and escaped
punctuation); ``.`` (any character but newline); classes ``[...]`` /
``[^...]`` with ranges; ``\\d \\w \\s`` (ASCII) and ``\\D \\W \\S``; groups
``(...)`` / ``(?:...)``; ``|``; ``? * +`` and ``{m} {m,} {m,n}`` (a trailing
lazy ``?`` is accepted: it does not change the language). Non-ASCII
literals match as their UTF-8 bytes; ``.`` and negated classes match whole
well-formed UTF-8 characters. Backreferences, lookaround, named groups,
inline flags, anchors and word boundaries raise ``ValueError``.

Supported JSON Schema subset: ``type`` object (``properties`` in declared
order, ``required`` mandatory, the rest optional, no additional
properties), array (``items``, ``minItems``, ``maxItems``), string
(``minLength``, ``maxLength``, ``pattern``), integer, number, boolean, null;
``enum``, ``const``, ``anyOf`` and non-recursive local ``$ref`` anywhere.
Whitespace: none, except one optional space after ``:`` and ``,``.
A schema with no constraint on a value (and ``json_object``) means any JSON
value whose containers nest at most ``json_depth`` deep -- a finite
automaton cannot count unbounded nesting (``{}`` has depth 1).

Measured cost (one CPU core): the largest schema of
tests/test_guided_cpu.py (BIG_SCHEMA) compiles in 40 ms (696 DFA states),
``json_object`` at depth 4 in 75-140 ms (1288 states); one state's mask over
a synthetic 128256-token byte-level vocabulary (tokens of 1-11 bytes) takes
4.3 ms including the bit packing. Compile time grows about linearly in
states, so the default ``max_states`` of 20000 bounds one to a few seconds.
"""

import json
import threading
from collections import OrderedDict
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np

ALL_BYTES = (1 << 256) - 1


def _mask_of(byte_values) -> int:
    m = 0
    for b in byte_values:
        m |= 1 << b
    return m


def _range_mask(lo: int, hi: int) -> int:
    return ((1 << (hi + 1)) - 1) & ~((1 << lo) - 1)


_DIGIT = _range_mask(0x30, 0x39)
_WORD = (_DIGIT | _range_mask(0x41, 0x5A) | _range_mask(0x61, 0x7A)
         | (1 << 0x5F))
_SPACE = _mask_of(b" \t\n\r\f\v")
_ASCII = _range_mask(0, 0x7F)
_CONT = _range_mask(0x80, 0xBF)


# --------------------------------------------------------------------- #
# regex AST: ("set", mask) one byte from a 256-bit set | ("cat", [nodes]) |
# ("alt", [nodes]) | ("rep", node, lo, hi|None) | ("seplist", item, sep):
# item (sep item)* built with ONE copy of item
# --------------------------------------------------------------------- #
def _cat(nodes):
    nodes = list(nodes)
    return nodes[0] if len(nodes) == 1 else ("cat", nodes)


def _alt(nodes):
    nodes = list(nodes)
    return nodes[0] if len(nodes) == 1 else ("alt", nodes)


def _lit(data) -> tuple:
    if isinstance(data, str):
        data = data.encode("utf-8")
    return ("cat", [("set", 1 << b) for b in data])


def _opt(node):
    return ("rep", node, 0, 1)


_EPS = ("cat", [])

# well-formed multi-byte UTF-8 (RFC 3629: no overlongs, no surrogates)
_UTF8_MULTI = _alt([
    _cat([("set", _range_mask(0xC2, 0xDF)), ("set", _CONT)]),
    _cat([("set", 1 << 0xE0), ("set", _range_mask(0xA0, 0xBF)),
          ("set", _CONT)]),
    _cat([("set", _range_mask(0xE1, 0xEC) | _range_mask(0xEE, 0xEF)),
          ("set", _CONT), ("set", _CONT)]),
    _cat([("set", 1 << 0xED), ("set", _range_mask(0x80, 0x9F)),
          ("set", _CONT)]),
    _cat([("set", 1 << 0xF0), ("set", _range_mask(0x90, 0xBF)),
          ("set", _CONT), ("set", _CONT)]),
    _cat([("set", _range_mask(0xF1, 0xF3)), ("set", _CONT), ("set", _CONT),
          ("set", _CONT)]),
    _cat([("set", 1 << 0xF4), ("set", _range_mask(0x80, 0x8F)),
          ("set", _CONT), ("set", _CONT)]),
])


def _char_class(ascii_mask: int, extra_chars=(), negate: bool = False):
    """One CHARACTER: ASCII members as a byte set, non-ASCII members as
    their UTF-8 sequences; a negated class also takes every multi-byte
    character (non-ASCII members cannot be subtracted from those)."""
    if negate:
        if extra_chars:
            raise ValueError("unsupported regex construct: non-ASCII "
                             "character inside a negated class")
        return _alt([("set", _ASCII & ~ascii_mask), _UTF8_MULTI])
    alts = [("set", ascii_mask)] if ascii_mask else []
    alts += [_lit(c) for c in extra_chars]
    if not alts:
        raise ValueError("regex: empty character class")
    return _alt(alts)


class _RegexParser:
    _SIMPLE_ESC = {"n": 10, "t": 9, "r": 13, "f": 12, "v": 11, "0": 0,
                   "a": 7}
    _CLASS_ESC = {"d": (_DIGIT, False), "D": (_DIGIT, True),
                  "w": (_WORD, False), "W": (_WORD, True),
                  "s": (_SPACE, False), "S": (_SPACE, True)}

    def __init__(self, pattern: str):
        if not isinstance(pattern, str):
            raise ValueError("regex must be a string")
        self.p = pattern
        self.i = 0

    def parse(self):
        node = self._alternation()
        if self.i < len(self.p):
            raise ValueError("regex: unbalanced ')' at {}".format(self.i))
        return node

    def _peek(self) -> Optional[str]:
        return self.p[self.i] if self.i < len(self.p) else None

    def _alternation(self):
        branches = [self._sequence()]
        while self._peek() == "|":
            self.i += 1
            branches.append(self._sequence())
        return _alt(branches)

    def _sequence(self):
        items = []
        while self._peek() is not None and self._peek() not in "|)":
            items.append(self._quantified())
        return _cat(items) if items else _EPS

    def _quantified(self):
        atom = self._atom()
        while True:
            c = self._peek()
            if c == "?":
                lo, hi = 0, 1
            elif c == "*":
                lo, hi = 0, None
            elif c == "+":
                lo, hi = 1, None
            elif c == "{":
                counted = self._count()
                if counted is None:
                    return atom
                lo, hi = counted
                self.i -= 1  # _count consumed through '}'
            else:
                return atom
            self.i += 1
            if self._peek() == "?":  # lazy: same language
                self.i += 1
            elif self._peek() == "+":
                raise ValueError("unsupported regex construct: possessive "
                                 "quantifier")
            atom = ("rep", atom, lo, hi)

    def _count(self) -> Optional[Tuple[int, Optional[int]]]:
        """``{m}``, ``{m,}``, ``{m,n}`` at self.i; None (nothing consumed)
        when the brace is a literal, as in ``re``."""
        end = self.p.find("}", self.i)
        if end < 0:
            return None
        body = self.p[self.i + 1:end]
        lo_s, comma, hi_s = body.partition(",")
        if (lo_s and not lo_s.isdigit()) or (hi_s and not hi_s.isdigit()) \
                or not (lo_s or hi_s):
            return None
        lo = int(lo_s) if lo_s else 0  # {,n} is {0,n}, as in ``re``
        hi = lo if not comma else (int(hi_s) if hi_s else None)
        if hi is not None and hi < lo:
            raise ValueError("regex: bad repeat {{{}}}".format(body))
        if max(lo, hi or 0) > 1000:
            raise ValueError("regex: repeat count above 1000 is too complex")
        self.i = end + 1
        return lo, hi

    def _atom(self):
        c = self._peek()
        self.i += 1
        if c == "(":
            if self._peek() == "?":
                nxt = self.p[self.i + 1:self.i + 2]
                if nxt == ":":
                    self.i += 2
                elif nxt in ("=", "!") or self.p[self.i + 1:self.i + 3] in (
                        "<=", "<!"):
                    raise ValueError("unsupported regex construct: "
                                     "lookaround")
                elif nxt == "P" or nxt == "<":
                    raise ValueError("unsupported regex construct: named "
                                     "group / named backreference")
                else:
                    raise ValueError("unsupported regex construct: inline "
                                     "flags / (?{}...)".format(nxt))
            node = self._alternation()
            if self._peek() != ")":
                raise ValueError("regex: missing ')'")
            self.i += 1
            return node
        if c == "[":
            return self._class()
        if c == ".":
            return _char_class(1 << 10, negate=True)
        if c in "^$":
            raise ValueError("unsupported regex construct: anchor '{}' "
                             "(matching is always a full match)".format(c))
        if c in "*+?":
            raise ValueError("regex: nothing to repeat at {}".format(
                self.i - 1))
        if c == "\\":
            kind, val = self._escape(in_class=False)
            if kind == "class":
                return _char_class(val[0], negate=val[1])
            return _lit(val)
        return _lit(c)

    def _escape(self, in_class: bool):
        """After a backslash -> ("char", str) | ("class", (mask, negate))."""
        c = self._peek()
        if c is None:
            raise ValueError("regex: trailing backslash")
        self.i += 1
        if c in self._CLASS_ESC:
            return "class", self._CLASS_ESC[c]
        if c == "b" and in_class:
            return "char", "\b"
        if c in "bBAZzG":
            raise ValueError("unsupported regex construct: anchor / word "
                             "boundary '\\{}'".format(c))
        if c in "123456789" or c in "kg":
            raise ValueError("unsupported regex construct: backreference "
                             "'\\{}'".format(c))
        if c in self._SIMPLE_ESC:
            return "char", chr(self._SIMPLE_ESC[c])
        if c in "xuU":
            n = {"x": 2, "u": 4, "U": 8}[c]
            digits = self.p[self.i:self.i + n]
            try:
                if len(digits) != n:
                    raise ValueError
                ch = chr(int(digits, 16))
                ch.encode("utf-8")
            except (ValueError, OverflowError):
                raise ValueError("regex: bad \\{} escape".format(c))
            self.i += n
            return "char", ch
        if c.isalnum():
            raise ValueError("unsupported regex construct: escape "
                             "'\\{}'".format(c))
        return "char", c

    def _class(self):
        negate = self._peek() == "^"
        if negate:
            self.i += 1
        mask = 0
        extra: List[str] = []
        multi = False
        first = True
        while True:
            c = self._peek()
            if c is None:
                raise ValueError("regex: missing ']'")
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            lo = self._class_char()
            if isinstance(lo, tuple):  # \d etc. inside a class
                m, neg = lo
                if neg:
                    if negate:
                        raise ValueError(
                            "unsupported regex construct: negated escape "
                            "inside a negated class")
                    mask |= _ASCII & ~m
                    multi = True
                else:
                    mask |= m
                continue
            if self._peek() == "-" and self.p[self.i + 1:self.i + 2] not in (
                    "]", ""):
                self.i += 1
                hi = self._class_char()
                if isinstance(hi, tuple):
                    raise ValueError("regex: bad character range")
                if ord(hi) < ord(lo):
                    raise ValueError("regex: bad character range {}-{}"
                                     .format(lo, hi))
                if ord(hi) > 0x7F:
                    raise ValueError("unsupported regex construct: "
                                     "non-ASCII character range")
                mask |= _range_mask(ord(lo), ord(hi))
            elif ord(lo) <= 0x7F:
                mask |= 1 << ord(lo)
            else:
                extra.append(lo)
        if multi:  # a \D \W \S member: every multi-byte character too
            alts = [("set", mask)] if mask else []
            return _alt(alts + [_UTF8_MULTI])
        return _char_class(mask, extra, negate)

    def _class_char(self):
        c = self._peek()
        self.i += 1
        if c == "\\":
            kind, val = self._escape(in_class=True)
            return val
        return c


def parse_regex(pattern: str):
    return _RegexParser(pattern).parse()


# --------------------------------------------------------------------- #
# AST -> NFA -> DFA
# --------------------------------------------------------------------- #
class _Nfa:
    def __init__(self, limit: int):
        self.eps: List[List[int]] = []
        self.edges: List[List[Tuple[int, int]]] = []  # (byte mask, target)
        self.limit = limit

    def state(self) -> int:
        if len(self.eps) >= self.limit:
            raise ValueError("grammar too complex: more than {} NFA states"
                             .format(self.limit))
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def build(self, node) -> Tuple[int, int]:
        kind = node[0]
        if kind == "set":
            s, e = self.state(), self.state()
            self.edges[s].append((node[1], e))
            return s, e
        if kind == "cat":
            s = cur = self.state()
            for child in node[1]:
                cs, ce = self.build(child)
                self.eps[cur].append(cs)
                cur = ce
            return s, cur
        if kind == "alt":
            s, e = self.state(), self.state()
            for child in node[1]:
                cs, ce = self.build(child)
                self.eps[s].append(cs)
                self.eps[ce].append(e)
            return s, e
        if kind == "seplist":
            s, e = self.state(), self.state()
            is_, ie = self.build(node[1])
            ss, se = self.build(node[2])
            self.eps[s].append(is_)
            self.eps[ie].append(e)
            self.eps[ie].append(ss)
            self.eps[se].append(is_)
            return s, e
        if kind == "rep":
            _, child, lo, hi = node
            s = cur = self.state()
            for _i in range(lo):
                cs, ce = self.build(child)
                self.eps[cur].append(cs)
                cur = ce
            if hi is None:
                cs, ce = self.build(child)
                loop = self.state()
                self.eps[cur].append(loop)
                self.eps[loop].append(cs)
                self.eps[ce].append(loop)
                return s, loop
            e = self.state()
            self.eps[cur].append(e)
            for _i in range(hi - lo):
                cs, ce = self.build(child)
                self.eps[cur].append(cs)
                self.eps[ce].append(e)
                cur = ce
            return s, e
        raise AssertionError(kind)


class Dfa:
    """trans: int32 [n_states + 1, 256]; the extra last row is the dead
    sink (every byte maps to itself), so a vectorised walk never indexes
    out of range. accept: bool [n_states + 1]. State 0 is the start."""

    def __init__(self, trans: np.ndarray, accept: np.ndarray):
        self.trans = trans
        self.accept = accept
        self.n_states = trans.shape[0] - 1
        self.dead = self.n_states

    def step(self, state: int, data: bytes) -> int:
        for b in data:
            state = int(self.trans[state, b])
        return state

    def matches(self, data) -> bool:
        if isinstance(data, str):
            data = data.encode("utf-8")
        return bool(self.accept[self.step(0, data)])


def compile_ast(ast, max_states: int = 20000) -> Dfa:
    nfa = _Nfa(limit=max(64 * max_states, 1 << 16))
    start, end = nfa.build(ast)
    n = len(nfa.eps)

    # byte equivalence classes: bytes no edge set tells apart move together
    sig: Dict[int, List[int]] = {}
    masks = {m for edges in nfa.edges for m, _t in edges}
    for b in range(256):
        key = 0
        for k, m in enumerate(masks):
            if (m >> b) & 1:
                key |= 1 << k
        sig.setdefault(key, []).append(b)
    classes = [bs for key, bs in sig.items() if key]  # key 0: no edge at all

    closure_cache: Dict[int, frozenset] = {}

    def closure(states) -> frozenset:
        out = set()
        stack = list(states)
        while stack:
            s = stack.pop()
            if s in out:
                continue
            cached = closure_cache.get(s)
            if cached is not None:
                out |= cached
                continue
            out.add(s)
            stack.extend(nfa.eps[s])
        return frozenset(out)

    start_set = closure([start])
    ids: Dict[frozenset, int] = {start_set: 0}
    order = [start_set]
    rows: List[Dict[int, int]] = []  # per DFA state: class index -> target
    target_closure: Dict[int, frozenset] = {}
    i = 0
    while i < len(order):
        cur = order[i]
        i += 1
        row: Dict[int, int] = {}
        live_edges = [(m, t) for s in cur for m, t in nfa.edges[s]]
        if live_edges:
            for ci, bs in enumerate(classes):
                bit = 1 << bs[0]
                targets = [t for m, t in live_edges if m & bit]
                if not targets:
                    continue
                nxt = set()
                for t in targets:
                    c = target_closure.get(t)
                    if c is None:
                        c = target_closure[t] = closure([t])
                    nxt |= c
                nxt = frozenset(nxt)
                j = ids.get(nxt)
                if j is None:
                    if len(order) >= max_states:
                        raise ValueError(
                            "grammar too complex: more than {} DFA states "
                            "(raise guided_max_states or simplify the "
                            "constraint)".format(max_states))
                    j = ids[nxt] = len(order)
                    order.append(nxt)
                row[ci] = j
        rows.append(row)

    ns = len(order)
    accept = np.zeros(ns, dtype=bool)
    for j, st in enumerate(order):
        accept[j] = end in st
    # prune dead states: keep only states that can reach an accepting one
    preds: List[List[int]] = [[] for _ in range(ns)]
    for j, row in enumerate(rows):
        for t in set(row.values()):
            preds[t].append(j)
    live = np.zeros(ns, dtype=bool)
    stack = [j for j in range(ns) if accept[j]]
    for j in stack:
        live[j] = True
    while stack:
        j = stack.pop()
        for p in preds[j]:
            if not live[p]:
                live[p] = True
                stack.append(p)
    if not live[0]:
        raise ValueError("the constraint matches no string at all")
    remap = np.full(ns, -1, dtype=np.int64)
    remap[live] = np.arange(int(live.sum()))
    nl = int(live.sum())
    trans = np.full((nl + 1, 256), nl, dtype=np.int32)
    for j, row in enumerate(rows):
        if not live[j]:
            continue
        for ci, t in row.items():
            if live[t]:
                trans[remap[j], classes[ci]] = remap[t]
    acc = np.zeros(nl + 1, dtype=bool)
    acc[:nl] = accept[live]
    return Dfa(trans, acc)


def compile_regex(pattern: str, max_states: int = 20000) -> Dfa:
    return compile_ast(parse_regex(pattern), max_states)


# --------------------------------------------------------------------- #
# JSON schema -> AST
# --------------------------------------------------------------------- #
_WS = _opt(("set", 1 << 0x20))  # the one optional space after ':' and ','
_COMMA = _cat([("set", 1 << 0x2C), _WS])
_COLON = _cat([("set", 1 << 0x3A), _WS])
_HEX = _DIGIT | _range_mask(0x41, 0x46) | _range_mask(0x61, 0x66)
# one string character: unescaped (no quote, backslash, control), a simple
# escape, or \uXXXX outside the surrogate range (so one alternative is
# exactly one code point and minLength/maxLength count correctly)
_STR_CHAR = _alt([
    _char_class(_range_mask(0, 0x1F) | (1 << 0x22) | (1 << 0x5C),
                negate=True),
    _cat([("set", 1 << 0x5C), _alt([
        ("set", _mask_of(b'"\\/bfnrt')),
        _cat([("set", 1 << 0x75), _alt([
            _cat([("set", _HEX & ~_mask_of(b"dD")), ("set", _HEX),
                  ("set", _HEX), ("set", _HEX)]),
            _cat([("set", _mask_of(b"dD")), ("set", _range_mask(0x30, 0x37)),
                  ("set", _HEX), ("set", _HEX)]),
        ])]),
    ])]),
])
_QUOTE = ("set", 1 << 0x22)
_INTEGER = _cat([_opt(("set", 1 << 0x2D)), _alt([
    ("set", 1 << 0x30),
    _cat([("set", _range_mask(0x31, 0x39)), ("rep", ("set", _DIGIT), 0, None)]),
])])
_NUMBER = _cat([
    _INTEGER,
    _opt(_cat([("set", 1 << 0x2E), ("rep", ("set", _DIGIT), 1, None)])),
    _opt(_cat([("set", _mask_of(b"eE")), _opt(("set", _mask_of(b"+-"))),
               ("rep", ("set", _DIGIT), 1, None)])),
])

_IGNORED_KEYS = {"title", "description", "default", "examples", "$schema",
                 "$id", "$defs", "definitions", "additionalProperties",
                 "$comment", "deprecated", "readOnly", "writeOnly", "format"}
_HANDLED_KEYS = {"type", "properties", "required", "items", "minItems",
                 "maxItems", "minLength", "maxLength", "pattern", "enum",
                 "const", "anyOf", "$ref"}
_REFUSED_KEYS = {"oneOf", "allOf", "not", "patternProperties", "if", "then",
                 "else", "minimum", "maximum", "exclusiveMinimum",
                 "exclusiveMaximum", "multipleOf", "uniqueItems",
                 "minProperties", "maxProperties", "prefixItems", "contains",
                 "propertyNames", "dependentRequired", "dependentSchemas",
                 "unevaluatedProperties", "unevaluatedItems"}


def _string_ast(lo: int = 0, hi: Optional[int] = None):
    return _cat([_QUOTE, ("rep", _STR_CHAR, lo, hi), _QUOTE])


def _json_literal(value) -> tuple:
    return _lit(json.dumps(value, ensure_ascii=False,
                           separators=(",", ":")))


def _list_ast(item, lo: int, hi: Optional[int]):
    """item (, item)* with between lo and hi items, brackets excluded."""
    if hi is None:
        if lo <= 1:
            body = ("seplist", item, _COMMA)
            return body if lo == 1 else _opt(body)
        return _cat([item] + [_cat([_COMMA, item])] * (lo - 2)
                    + [_COMMA, ("seplist", item, _COMMA)])
    if hi == 0:
        return _EPS
    tail = _EPS
    for _i in range(hi - max(lo, 1)):  # optional items nest from the end
        tail = _opt(_cat([_COMMA, item, tail]))
    body = _cat([item] + [_cat([_COMMA, item])] * (max(lo, 1) - 1) + [tail])
    return body if lo >= 1 else _opt(body)


def json_value_ast(depth: int):
    """Any JSON value whose containers nest at most ``depth`` deep."""
    alts = [_string_ast(), _NUMBER, _lit("true"), _lit("false"),
            _lit("null")]
    if depth > 0:
        alts.append(json_object_ast(depth))
        alts.append(_cat([_lit("["),
                          _list_ast(json_value_ast(depth - 1), 0, None),
                          _lit("]")]))
    return _alt(alts)


def json_object_ast(depth: int):
    """Any JSON object of container depth <= ``depth`` (``{}`` is 1)."""
    if depth < 1:
        raise ValueError("guided_json_depth must be >= 1")
    pair = _cat([_string_ast(), _COLON, json_value_ast(depth - 1)])
    return _cat([_lit("{"), _list_ast(pair, 0, None), _lit("}")])


class _SchemaCompiler:
    def __init__(self, root: Any, depth: int):
        self.root = root
        self.depth = depth
        self.ref_stack: List[str] = []

    def _int(self, schema, key, default):
        v = schema.get(key, default)
        if v is None:
            return None
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError("schema: '{}' must be a non-negative integer"
                             .format(key))
        return v

    def compile(self, schema, depth: Optional[int] = None):
        depth = self.depth if depth is None else depth
        if schema is True or schema == {}:
            return json_value_ast(depth)
        if not isinstance(schema, dict):
            raise ValueError("schema must be an object, got {!r}".format(
                schema))
        for key in schema:
            if key in _REFUSED_KEYS:
                raise ValueError("unsupported schema keyword '{}'".format(
                    key))
        if "$ref" in schema:
            return self._ref(schema["$ref"], depth)
        if "const" in schema:
            return _json_literal(schema["const"])
        if "enum" in schema:
            if not isinstance(schema["enum"], list) or not schema["enum"]:
                raise ValueError("schema: 'enum' must be a non-empty list")
            return _alt([_json_literal(v) for v in schema["enum"]])
        if "anyOf" in schema:
            if not isinstance(schema["anyOf"], list) or not schema["anyOf"]:
                raise ValueError("schema: 'anyOf' must be a non-empty list")
            return _alt([self.compile(s, depth) for s in schema["anyOf"]])
        t = schema.get("type")
        if isinstance(t, list):
            return _alt([self.compile({**schema, "type": one}, depth)
                         for one in t])
        if t is None:
            if "properties" in schema:
                t = "object"
            elif "items" in schema:
                t = "array"
            elif "pattern" in schema or "maxLength" in schema \
                    or "minLength" in schema:
                t = "string"
            else:
                return json_value_ast(depth)
        if t == "string":
            if "pattern" in schema:
                if "minLength" in schema or "maxLength" in schema:
                    raise ValueError("schema: 'pattern' cannot be combined "
                                     "with minLength/maxLength")
                return _cat([_QUOTE, parse_regex(schema["pattern"]), _QUOTE])
            lo = self._int(schema, "minLength", 0)
            hi = self._int(schema, "maxLength", None)
            if hi is not None and hi < lo:
                raise ValueError("schema: maxLength < minLength")
            return _string_ast(lo, hi)
        if t == "integer":
            return _INTEGER
        if t == "number":
            return _NUMBER
        if t == "boolean":
            return _alt([_lit("true"), _lit("false")])
        if t == "null":
            return _lit("null")
        if t == "array":
            lo = self._int(schema, "minItems", 0)
            hi = self._int(schema, "maxItems", None)
            if hi is not None and hi < lo:
                raise ValueError("schema: maxItems < minItems")
            item = self.compile(schema.get("items", True), max(depth - 1, 0))
            return _cat([_lit("["), _list_ast(item, lo, hi), _lit("]")])
        if t == "object":
            props = schema.get("properties")
            if props is None:
                return json_object_ast(max(depth, 1))
            if not isinstance(props, dict):
                raise ValueError("schema: 'properties' must be an object")
            required = schema.get("required") or []
            unknown = [r for r in required if r not in props]
            if unknown:
                raise ValueError("schema: required key(s) {} have no entry "
                                 "in 'properties'".format(unknown))
            return self._object(list(props.items()), set(required), depth)
        raise ValueError("unsupported schema type {!r}".format(t))

    def _object(self, props, required, depth):
        pairs = [_cat([_json_literal(k), _COLON,
                       self.compile(sub, max(depth - 1, 0))])
                 for k, sub in props]
        n = len(pairs)
        # after[i]: properties i.. when one was already emitted (each takes
        # its own leading comma); first[i]: properties i.. when none was
        after = [None] * (n + 1)
        first = [None] * (n + 1)
        after[n] = first[n] = _EPS
        for i in range(n - 1, -1, -1):
            with_comma = _cat([_COMMA, pairs[i]])
            if props[i][0] in required:
                after[i] = _cat([with_comma, after[i + 1]])
                first[i] = _cat([pairs[i], after[i + 1]])
            else:
                after[i] = _cat([_opt(with_comma), after[i + 1]])
                first[i] = _alt([_cat([pairs[i], after[i + 1]]),
                                 first[i + 1]])
        return _cat([_lit("{"), first[0], _lit("}")])

    def _ref(self, ref, depth):
        if not isinstance(ref, str) or not ref.startswith("#/"):
            raise ValueError("unsupported $ref {!r}: only local '#/$defs/"
                             "...' references".format(ref))
        if ref in self.ref_stack:
            raise ValueError("recursive $ref {!r} is not supported (a "
                             "finite automaton cannot nest without bound)"
                             .format(ref))
        node = self.root
        for part in ref[2:].split("/"):
            part = part.replace("~1", "/").replace("~0", "~")
            if not isinstance(node, dict) or part not in node:
                raise ValueError("unresolvable $ref {!r}".format(ref))
            node = node[part]
        self.ref_stack.append(ref)
        try:
            return self.compile(node, depth)
        finally:
            self.ref_stack.pop()


def schema_ast(schema: Any, depth: int = 4):
    return _SchemaCompiler(schema, depth).compile(schema)


# --------------------------------------------------------------------- #
# vocabulary as bytes
# --------------------------------------------------------------------- #
def _gpt2_unicode_to_byte() -> Dict[str, int]:
    """Inverse of the GPT-2 byte<->unicode table every ByteLevel BPE uses."""
    keep = (list(range(ord("!"), ord("~") + 1))
            + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1)))
    table = {chr(b): b for b in keep}
    extra = 0
    for b in range(256):
        if b not in keep:
            table[chr(256 + extra)] = b
            extra += 1
    return table


def _has_bytelevel(node) -> bool:
    if isinstance(node, dict):
        if node.get("type") == "ByteLevel":
            return True
        return any(_has_bytelevel(v) for v in node.values())
    if isinstance(node, list):
        return any(_has_bytelevel(v) for v in node)
    return False


def token_bytes_of(tokenizer) -> List[Optional[bytes]]:
    """Per token id, the bytes it appends to the output (None = none:
    special/added tokens). Raises ValueError for tokenizers whose tokens
    are not byte strings."""
    hf = getattr(tokenizer, "_tok", None)
    if hf is None:
        if getattr(tokenizer, "vocab_size", None) == 257 \
                and hasattr(tokenizer, "encode") \
                and tokenizer.encode("A") == [66]:
            return [None] + [bytes([i]) for i in range(256)]
        raise ValueError("guided_decoding does not support tokenizer {!r}"
                         .format(type(tokenizer).__name__))
    spec = json.loads(hf.to_str())
    if not (_has_bytelevel(spec.get("pre_tokenizer"))
            or _has_bytelevel(spec.get("decoder"))):
        raise ValueError(
            "guided_decoding needs a byte-level BPE tokenizer (ByteLevel "
            "pre-tokenizer/decoder, as llama-3 / qwen2 / gpt2) or the "
            "built-in byte tokenizer; this tokenizer.json has neither")
    u2b = _gpt2_unicode_to_byte()
    added = {int(t["id"]) for t in spec.get("added_tokens") or []}
    vocab = hf.get_vocab(with_added_tokens=True)
    out: List[Optional[bytes]] = [None] * (max(vocab.values()) + 1
                                           if vocab else 0)
    for tok, tid in vocab.items():
        if tid in added:
            continue
        try:
            out[tid] = bytes(u2b[ch] for ch in tok)
        except KeyError:
            pass  # not a byte-level token string: never allowed
    return out


class Vocabulary:
    """The token vocabulary as a padded byte matrix, sorted by length so the
    lock-step DFA walk only touches tokens that still have bytes left."""

    def __init__(self, token_bytes: List[Optional[bytes]], width: int,
                 eos_id: int):
        self.width = int(width)              # V: the model's logits width
        self.words = (self.width + 31) // 32
        self.eos_id = int(eos_id)
        self.token_bytes: List[Optional[bytes]] = [
            (b if b and i != eos_id else None)
            for i, b in enumerate(token_bytes[:self.width])]
        ids = [i for i, b in enumerate(self.token_bytes) if b]
        ids.sort(key=lambda i: -len(self.token_bytes[i]))
        self.ids = np.asarray(ids, dtype=np.int64)
        lmax = len(self.token_bytes[ids[0]]) if ids else 0
        self.mat = np.zeros((len(ids), lmax), dtype=np.uint8)
        lens = np.zeros(len(ids), dtype=np.int64)
        for r, i in enumerate(ids):
            b = self.token_bytes[i]
            self.mat[r, :len(b)] = np.frombuffer(b, dtype=np.uint8)
            lens[r] = len(b)
        # active[j]: number of (length-sorted) tokens with more than j bytes
        self.active = [int((lens > j).sum()) for j in range(lmax)]
        self.mat = np.ascontiguousarray(self.mat.T)  # [Lmax, n] column walk

    def allowed(self, dfa: Dfa, state: int) -> np.ndarray:
        """bool [width]: tokens whose bytes stay inside live states."""
        cur = np.full(len(self.ids), state, dtype=np.int32)
        for j, n in enumerate(self.active):
            cur[:n] = dfa.trans[cur[:n], self.mat[j, :n]]
        out = np.zeros(self.words * 32, dtype=bool)
        out[self.ids[cur != dfa.dead]] = True
        return out


def pack_bits(allowed: np.ndarray) -> np.ndarray:
    """bool [W*32] -> int32 [W]; token t is bit t&31 of word t>>5."""
    return np.packbits(allowed, bitorder="little").view("<u4").astype(
        np.uint32).view(np.int32)


# --------------------------------------------------------------------- #
# compiled grammar, per-sequence state, compile cache
# --------------------------------------------------------------------- #
class Grammar:
    _next_uid = [0]

    def __init__(self, dfa: Dfa, vocab: Vocabulary, key: str):
        self.dfa = dfa
        self.vocab = vocab
        self.key = key
        Grammar._next_uid[0] += 1
        self.uid = Grammar._next_uid[0]
        # state -> (bool allowed[W*32] with no eos/stop bit, count)
        self._masks: Dict[int, Tuple[np.ndarray, int]] = {}
        self._lock = threading.Lock()

    def token_mask(self, state: int) -> Tuple[np.ndarray, int]:
        """(allowed byte tokens of ``state``, how many); lazily computed,
        cached for the life of the grammar."""
        hit = self._masks.get(state)
        if hit is None:
            with self._lock:
                hit = self._masks.get(state)
                if hit is None:
                    allowed = self.vocab.allowed(self.dfa, state)
                    hit = self._masks[state] = (allowed, int(allowed.sum()))
        return hit


class GuidedState:
    """One sequence's position in its grammar. ``stop_ids`` (eos + the
    request's stop_token_ids) are allowed iff the state is accepting --
    and ONLY then, since emitting one finishes the sequence."""

    def __init__(self, grammar: Grammar, stop_ids=()):
        self.grammar = grammar
        self.state = 0
        v = grammar.vocab
        self.stop_ids = tuple(sorted({int(t) for t in stop_ids
                                      if 0 <= int(t) < v.width}))

    @property
    def key(self) -> tuple:
        """Identity of mask_words(): the MaskBank slot key."""
        return (self.grammar.uid, self.state, self.stop_ids)

    @property
    def dead(self) -> bool:
        return self.state == self.grammar.dfa.dead

    def accepting(self) -> bool:
        return bool(self.grammar.dfa.accept[self.state])

    def advance(self, token_id: int) -> None:
        if token_id in self.stop_ids:
            return  # finishing token: the state is final as it stands
        data = (self.grammar.vocab.token_bytes[token_id]
                if 0 <= token_id < self.grammar.vocab.width else None)
        self.state = (self.grammar.dfa.step(self.state, data) if data
                      else self.grammar.dfa.dead)

    def _allowed(self) -> np.ndarray:
        allowed, _n = self.grammar.token_mask(self.state)
        if self.stop_ids:
            allowed = allowed.copy()
            allowed[list(self.stop_ids)] = self.accepting()
        return allowed

    def num_continuations(self) -> int:
        """Allowed tokens that do NOT finish the sequence."""
        if self.dead:
            return 0
        allowed, n = self.grammar.token_mask(self.state)
        return n - int(allowed[list(self.stop_ids)].sum())

    def num_allowed(self) -> int:
        if self.dead:
            return 0
        return self.num_continuations() + (len(self.stop_ids)
                                           if self.accepting() else 0)

    def allows(self, token_id: int) -> bool:
        return (not self.dead and 0 <= token_id < self.grammar.vocab.width
                and bool(self._allowed()[token_id]))

    def mask_words(self) -> np.ndarray:
        """int32 [W] packed mask of the current state."""
        if self.dead:
            return np.zeros(self.grammar.vocab.words, dtype=np.int32)
        return pack_bits(self._allowed())


def canonical_spec(kind: str, spec: Any) -> Tuple[str, Any, str]:
    """Validate + normalise a request constraint -> (kind, spec, key)."""
    if kind == "json":
        if isinstance(spec, str):
            try:
                spec = json.loads(spec)
            except ValueError:
                raise ValueError("guided_json is not valid JSON")
        if not isinstance(spec, (dict, bool)):
            raise ValueError("guided_json must be a JSON schema object")
        key = json.dumps(spec, sort_keys=False, separators=(",", ":"))
    elif kind == "regex":
        if not isinstance(spec, str) or not spec:
            raise ValueError("guided_regex must be a non-empty string")
        key = spec
    elif kind == "choice":
        if not isinstance(spec, (list, tuple)) or not spec \
                or not all(isinstance(c, str) and c for c in spec):
            raise ValueError("guided_choice must be a non-empty list of "
                             "non-empty strings")
        spec = list(spec)
        key = json.dumps(spec)
    elif kind == "json_object":
        spec, key = None, ""
    else:
        raise ValueError("unknown guided-decoding kind {!r}".format(kind))
    return kind, spec, "{}:{}".format(kind, key)


class GuidedCompiler:
    """Constraint -> Grammar for one engine's vocabulary, with an LRU of
    compiled grammars keyed by the canonical spec."""

    def __init__(self, tokenizer, logits_width: int, max_states: int = 20000,
                 json_depth: int = 4, cache_size: int = 64):
        self.vocab = Vocabulary(token_bytes_of(tokenizer), logits_width,
                                tokenizer.eos_id)
        self.max_states = int(max_states)
        self.json_depth = int(json_depth)
        if self.json_depth < 1:
            raise ValueError("guided_json_depth must be >= 1")
        self.cache_size = cache_size
        self._cache: "OrderedDict[str, Grammar]" = OrderedDict()
        self._lock = threading.Lock()

    def ast(self, kind: str, spec: Any):
        if kind == "regex":
            return parse_regex(spec)
        if kind == "choice":
            return _alt([_lit(c) for c in spec])
        if kind == "json_object":
            return json_object_ast(self.json_depth)
        return schema_ast(spec, self.json_depth)

    def compile(self, kind: str, spec: Any) -> Grammar:
        kind, spec, key = canonical_spec(kind, spec)
        with self._lock:
            hit = self._cache.get(key)
            if hit is not None:
                self._cache.move_to_end(key)
                return hit
        try:
            dfa = compile_ast(self.ast(kind, spec), self.max_states)
        except RecursionError:
            raise ValueError("grammar too complex: nesting too deep")
        grammar = Grammar(dfa, self.vocab, key)
        with self._lock:
            self._cache[key] = grammar
            while len(self._cache) > self.cache_size:
                self._cache.popitem(last=False)
        return grammar


# --------------------------------------------------------------------- #
# request parsing
# --------------------------------------------------------------------- #
GUIDED_FIELDS = ("guided_json", "guided_regex", "guided_choice",
                 "structured_outputs")


def constraint_from_request(body: Dict[str, Any]
                            ) -> Optional[Tuple[str, Any]]:
    """The one guided-decoding constraint of a request body, as (kind,
    spec), or None. More than one is a ValueError."""
    found: List[Tuple[str, Any]] = []
    rf = body.get("response_format")
    if rf and isinstance(rf, dict) and rf.get("type") not in (None, "text"):
        if rf["type"] == "json_object":
            found.append(("json_object", None))
        elif rf["type"] == "json_schema":
            js = rf.get("json_schema")
            if not isinstance(js, dict) or "schema" not in js:
                raise ValueError("response_format json_schema needs "
                                 "{'json_schema': {'schema': {...}}}")
            found.append(("json", js["schema"]))
        else:
            raise ValueError("response_format type '{}' is not supported "
                             "(have: text, json_object, json_schema)"
                             .format(rf["type"]))
    for field, kind in (("guided_json", "json"), ("guided_regex", "regex"),
                        ("guided_choice", "choice")):
        if body.get(field) is not None:
            found.append((kind, body[field]))
    so = body.get("structured_outputs")
    if so is not None:
        if not isinstance(so, dict):
            raise ValueError("'structured_outputs' must be an object")
        for k, v in so.items():
            if k not in ("json", "regex", "choice"):
                raise ValueError("structured_outputs key '{}' is not "
                                 "supported (have: json, regex, choice)"
                                 .format(k))
            if v is not None:
                found.append((k, v))
    if len(found) > 1:
        raise ValueError("a request takes at most one guided-decoding "
                         "constraint, got {}".format(
                             [k for k, _ in found]))
    if not found:
        return None
    kind, spec, _key = canonical_spec(*found[0])
    return kind, spec


# --------------------------------------------------------------------- #
# device-side mask bank
# --------------------------------------------------------------------- #
class MaskBank:
    """[slots, W] int32 masks on the engine's device, the operand of the
    token_mask kernels. Slots are keyed by GuidedState.key with LRU
    eviction that never takes a slot the current step uses; a miss is one
    row copy from a pinned host mirror.

    The host row of a slot is rewritten only on a later miss for that slot;
    every sampling step ends in a device->host read of the sampled ids, so
    the previous async copy out of that row has long completed."""

    def __init__(self, slots: int, words: int, device, stats: Dict[str, int]):
        import torch

        self.slots = int(slots)
        self.bank = torch.zeros(self.slots, words, dtype=torch.int32,
                                device=device)
        pin = getattr(device, "type", str(device)) == "cuda"
        self.host = torch.zeros(self.slots, words, dtype=torch.int32,
                                pin_memory=pin)
        self._lru: "OrderedDict[tuple, int]" = OrderedDict()
        self._free = list(range(self.slots - 1, -1, -1))
        self._step: set = set()
        self.stats = stats

    def begin_step(self) -> None:
        self._step = set()

    def acquire(self, key: tuple, words_fn: Callable[[], np.ndarray]) -> int:
        import torch

        self._step.add(key)
        slot = self._lru.get(key)
        if slot is not None:
            self._lru.move_to_end(key)
            self.stats["guided_mask_hits"] += 1
            return slot
        self.stats["guided_mask_misses"] += 1
        if self._free:
            slot = self._free.pop()
        else:
            victim = next((k for k in self._lru if k not in self._step),
                          None)
            if victim is None:
                raise RuntimeError("guided mask bank exhausted within one "
                                   "step (guided_mask_slots < batch)")
            slot = self._lru.pop(victim)
        self.host[slot].copy_(torch.from_numpy(words_fn()))
        self.bank[slot].copy_(self.host[slot], non_blocking=True)
        self._lru[key] = slot
        return slot
