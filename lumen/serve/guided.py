"""Guided decoding: regex / choice / JSON-schema constraints compiled to a token table.

The pipeline is host only and pure Python + numpy / torch:

  pattern --parse--> AST --Thompson--> NFA --subset construction--> DFA over BYTES
          --minimise, trim--> ``trans`` int32 [S, 256] (-1 = dead), ``accept`` bool [S]
          --token bytes of the tokenizer--> ``next`` int16 [S, V]

``next[s][t]`` is the state after walking token t's bytes from state s, or -1 when the token is
not allowed there; ``next[s][eos] = s`` exactly for accepting s.  The sampling launch
(kernels/sampling_rows.hip) masks a guided row with its state's table row and advances the state
itself, so a guided request never needs token values on the host.

The match is always a full match.  ``guided_choice`` is an alternation of escaped literals and
``guided_json`` a schema lowered to a regex (``schema_to_regex``), so all three share one path.
Everything the compiler does not support raises ``ValueError`` naming the construct.
"""
from __future__ import annotations

import hashlib
import json
import re as _re
import time
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

# ---------------------------------------------------------------------------------------------
# regex subset -> AST.  Nodes: ("set", mask[256] bool) | ("cat", [nodes]) | ("alt", [nodes]) |
# ("rep", node, lo, hi or None)
# ---------------------------------------------------------------------------------------------
_META = set("\\.[]()|?*+{}^$")


def _mask(*ranges) -> np.ndarray:
    m = np.zeros(256, dtype=bool)
    for r in ranges:
        if isinstance(r, int):
            m[r] = True
        else:
            m[r[0]:r[1] + 1] = True
    return m


_DIGIT = _mask((0x30, 0x39))
_WORD = _mask((0x30, 0x39), (0x41, 0x5A), (0x61, 0x7A), 0x5F)
_SPACE = _mask(0x20, (0x09, 0x0D))
_CLASS_ESC = {"d": _DIGIT, "w": _WORD, "s": _SPACE, "D": ~_DIGIT, "W": ~_WORD, "S": ~_SPACE}
_CHAR_ESC = {"n": 0x0A, "t": 0x09, "r": 0x0D, "f": 0x0C, "v": 0x0B, "0": 0x00}
_QUANT = _re.compile(r"\{(\d+)(?:(,)(\d*))?\}")


def _lit(bs: bytes):
    nodes = [("set", _mask(b)) for b in bs]
    return nodes[0] if len(nodes) == 1 else ("cat", nodes)


class _Parser:
    def __init__(self, pattern: str):
        if not isinstance(pattern, str):
            raise ValueError("a regex must be a string")
        p = pattern
        if p.startswith("^"):
            p = p[1:]
        if p.endswith("$") and not _escaped_at(p, len(p) - 1):
            p = p[:-1]
        self.p, self.i = p, 0

    def fail(self, what: str):
        raise ValueError(f"unsupported regex construct: {what} (at offset {self.i} of "
                         f"{self.p!r})")

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.i < len(self.p) and self.p[self.i] == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.p[self.i] not in "|)":
            items.append(self.repeat())
        return ("cat", items)

    def repeat(self):
        node = self.atom()
        quantified = False
        while self.i < len(self.p):
            c = self.p[self.i]
            m = _QUANT.match(self.p, self.i) if c == "{" else None
            if c in "?*+":
                lo, hi = {"?": (0, 1), "*": (0, None), "+": (1, None)}[c]
                self.i += 1
            elif m:
                lo = int(m.group(1))
                hi = lo if m.group(2) is None else (int(m.group(3)) if m.group(3) else None)
                if hi is not None and hi < lo:
                    self.fail("repeat {m,n} with n < m")
                if max(lo, hi or 0) > 1000:
                    self.fail("repeat count above 1000")
                self.i = m.end()
            else:
                break
            if quantified:
                self.fail("a quantifier on a quantifier (possessive or multiple repeat)")
            quantified = True
            node = ("rep", node, lo, hi)
            if self.i < len(self.p) and self.p[self.i] == "?":
                self.i += 1  # lazy form: the same language
        return node

    def atom(self):
        c = self.p[self.i]
        if c == "(":
            self.i += 1
            if self.p.startswith("?", self.i):
                if self.p.startswith("?:", self.i):
                    self.i += 2
                elif self.p.startswith(("?=", "?!", "?<=", "?<!"), self.i):
                    self.fail("lookaround")
                elif self.p.startswith("?P=", self.i):
                    self.fail("backreference")
                elif self.p.startswith(("?P<", "?<"), self.i):
                    self.fail("named group")
                else:
                    self.fail("inline flags / group extension")
            node = self.alt()
            if self.i >= len(self.p) or self.p[self.i] != ")":
                self.fail("unbalanced '('")
            self.i += 1
            return node
        if c == "[":
            return self.cls()
        if c == ".":
            self.i += 1
            m = np.ones(256, dtype=bool)
            m[0x0A] = False
            return ("set", m)
        if c == "\\":
            kind, v = self.escape()
            return ("set", v) if kind == "set" else ("set", _mask(v))
        if c in "^$":
            self.fail(f"anchor '{c}' inside the pattern")
        if c in "?*+":
            self.fail("quantifier with nothing to repeat")
        self.i += 1
        return _lit(c.encode("utf-8"))

    def escape(self) -> Tuple[str, object]:
        """After a backslash: ("set", mask) or ("byte", value)."""
        self.i += 1
        if self.i >= len(self.p):
            self.fail("trailing backslash")
        c = self.p[self.i]
        self.i += 1
        if c in _CLASS_ESC:
            return "set", _CLASS_ESC[c].copy()
        if c == "x":
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or not all(x in "0123456789abcdefABCDEF" for x in h):
                self.fail("\\x needs two hex digits")
            self.i += 2
            return "byte", int(h, 16)
        if c in _CHAR_ESC:
            return "byte", _CHAR_ESC[c]
        if c.isdigit():
            self.fail("backreference")
        if c in "bBAZzG":
            self.fail(f"anchor '\\{c}' inside the pattern")
        if c.isalnum() or ord(c) > 127:
            self.fail(f"escape '\\{c}'")
        return "byte", ord(c)

    def cls(self):
        self.i += 1
        neg = self.p.startswith("^", self.i)
        if neg:
            self.i += 1
        m = np.zeros(256, dtype=bool)
        multi: List[bytes] = []
        first = True
        while True:
            if self.i >= len(self.p):
                self.fail("unbalanced '['")
            c = self.p[self.i]
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            lo = self._cls_item(m, multi)
            if lo is None:
                continue
            if (self.p.startswith("-", self.i) and self.i + 1 < len(self.p)
                    and self.p[self.i + 1] != "]"):
                self.i += 1
                hi = self._cls_item(None, None)
                if hi is None or hi < lo:
                    self.fail("bad class range")
                m[lo:hi + 1] = True
            else:
                m[lo] = True
        if neg:
            if multi:
                self.fail("non-ASCII character in a negated class")
            return ("set", ~m)
        if not multi:
            return ("set", m)
        return ("alt", ([("set", m)] if m.any() else []) + [_lit(b) for b in multi])

    def _cls_item(self, m, multi) -> Optional[int]:
        """One class member: its byte value, or None when it was a set / multi-byte literal
        (added to ``m`` / ``multi``, which are None where a range end is parsed)."""
        c = self.p[self.i]
        if c == "\\":
            kind, v = self.escape()
            if kind == "set":
                if m is None:
                    self.fail("bad class range")
                m |= v
                return None
            return v
        if c == "[" and self.p.startswith("[:", self.i):
            self.fail("POSIX class")
        self.i += 1
        if ord(c) > 127:
            if multi is None:
                self.fail("non-ASCII class range")
            multi.append(c.encode("utf-8"))
            return None
        return ord(c)


def _escaped_at(p: str, i: int) -> bool:
    n = 0
    while i - 1 - n >= 0 and p[i - 1 - n] == "\\":
        n += 1
    return n % 2 == 1


# ---------------------------------------------------------------------------------------------
# Thompson NFA -> DFA -> minimise -> trim
# ---------------------------------------------------------------------------------------------
class _NFA:
    def __init__(self):
        self.eps: List[List[int]] = []
        self.edge: List[Optional[Tuple[np.ndarray, int]]] = []   # at most one byte edge a state

    def new(self) -> int:
        self.eps.append([])
        self.edge.append(None)
        if len(self.eps) > 200000:
            raise ValueError("regex too large (more than 200000 NFA states)")
        return len(self.eps) - 1

    def build(self, node) -> Tuple[int, int]:
        k = node[0]
        if k == "set":
            a, b = self.new(), self.new()
            self.edge[a] = (node[1], b)
            return a, b
        if k == "cat":
            a = b = self.new()
            for n in node[1]:
                x, y = self.build(n)
                self.eps[b].append(x)
                b = y
            return a, b
        if k == "alt":
            a, b = self.new(), self.new()
            for n in node[1]:
                x, y = self.build(n)
                self.eps[a].append(x)
                self.eps[y].append(b)
            return a, b
        _, inner, lo, hi = node
        a = b = self.new()
        for _ in range(lo):
            x, y = self.build(inner)
            self.eps[b].append(x)
            b = y
        if hi is None:
            x, y = self.build(inner)
            loop = self.new()
            self.eps[b].append(loop)
            self.eps[loop].append(x)
            self.eps[y].append(loop)
            b = loop
        else:
            end = self.new()
            for _ in range(hi - lo):
                x, y = self.build(inner)
                self.eps[b].append(end)
                self.eps[b].append(x)
                b = y
            self.eps[b].append(end)
            b = end
        return a, b

    def closure(self, states) -> frozenset:
        seen = set(states)
        stack = list(states)
        while stack:
            for t in self.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)


def _subset(nfa: _NFA, start: int, final: int, max_states: int):
    s0 = nfa.closure([start])
    ids: Dict[frozenset, int] = {s0: 0}
    order = [s0]
    rows: List[np.ndarray] = []
    cl_cache: Dict[frozenset, frozenset] = {}
    i = 0
    while i < len(order):
        cur = order[i]
        i += 1
        row = np.full(256, -1, dtype=np.int32)
        edges = [nfa.edge[s] for s in cur if nfa.edge[s] is not None]
        if edges:
            M = np.stack([e[0] for e in edges])          # [E, 256]
            tg = [e[1] for e in edges]
            cols, inv = np.unique(M.T, axis=0, return_inverse=True)
            inv = inv.reshape(-1)
            for ci in range(cols.shape[0]):
                if not cols[ci].any():
                    continue
                raw = frozenset(tg[e] for e in np.nonzero(cols[ci])[0])
                nxt = cl_cache.get(raw)
                if nxt is None:
                    nxt = cl_cache[raw] = nfa.closure(raw)
                j = ids.get(nxt)
                if j is None:
                    j = ids[nxt] = len(order)
                    order.append(nxt)
                    if len(order) > 8 * max_states + 64:
                        raise ValueError(f"grammar needs more than {max_states} states "
                                         f"(--guided-max-states)")
                row[inv == ci] = j
        rows.append(row)
    trans = np.stack(rows)
    accept = np.fromiter((final in s for s in order), dtype=bool, count=len(order))
    return trans, accept


def _trim(trans: np.ndarray, accept: np.ndarray):
    """Drop states from which no accepting state is reachable, and those the start state does
    not reach; renumber in breadth-first order so the start state is 0."""
    S = trans.shape[0]
    good = accept.copy()
    while True:
        t = np.where(trans >= 0, good[np.maximum(trans, 0)], False).any(axis=1) | good
        if (t == good).all():
            break
        good = t
    if not good[0]:
        raise ValueError("the grammar matches nothing")
    trans = np.where((trans >= 0) & good[np.maximum(trans, 0)], trans, -1)
    new = np.full(S, -1, dtype=np.int64)
    new[0] = 0
    order = [0]
    i = 0
    while i < len(order):
        for t in np.unique(trans[order[i]]):
            if t >= 0 and new[t] < 0:
                new[t] = len(order)
                order.append(int(t))
        i += 1
    o = np.asarray(order)
    tr = trans[o]
    tr = np.where(tr >= 0, new[np.maximum(tr, 0)], -1).astype(np.int32)
    return tr, accept[o]


def _minimise(trans: np.ndarray, accept: np.ndarray):
    """Moore partition refinement; the start state's block becomes state 0 in ``_trim``."""
    S = trans.shape[0]
    lab = accept.astype(np.int64)
    n = len(np.unique(lab))
    while True:
        ext = np.concatenate([lab, [-1]])                     # index -1 (dead) -> label -1
        sig = np.concatenate([lab[:, None], ext[trans]], axis=1)
        _, first, inv = np.unique(sig, axis=0, return_index=True, return_inverse=True)
        inv = inv.reshape(-1)
        if len(first) == n:
            break
        n, lab = len(first), inv
    # blocks numbered by their smallest member keep state 0's block first
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    lab = rank[inv]
    rep = first[order]
    tr = trans[rep]
    tr = np.where(tr >= 0, lab[np.maximum(tr, 0)], -1).astype(np.int32)
    return tr, accept[rep]


def compile_regex(pattern: str, max_states: int = 4096) -> Tuple[np.ndarray, np.ndarray]:
    """(trans int32 [S, 256] with -1 = dead, accept bool [S]); state 0 is the start state and
    every state reaches an accepting one."""
    ast = _Parser(pattern).parse()
    nfa = _NFA()
    a, b = nfa.build(ast)
    trans, accept = _subset(nfa, a, b, max_states)
    trans, accept = _trim(trans, accept)
    trans, accept = _minimise(trans, accept)
    trans, accept = _trim(trans, accept)
    if trans.shape[0] > max_states:
        raise ValueError(f"grammar needs {trans.shape[0]} states, more than the limit of "
                         f"{max_states} (--guided-max-states)")
    return trans, accept


def dfa_matches(trans: np.ndarray, accept: np.ndarray, data: bytes) -> bool:
    s = 0
    for b in data:
        s = int(trans[s, b])
        if s < 0:
            return False
    return bool(accept[s])


def regex_escape(text: str) -> str:
    return "".join("\\" + c if c in _META else {"\n": "\\n", "\t": "\\t", "\r": "\\r"}.get(c, c)
                   for c in text)


def choice_to_regex(choices) -> str:
    if (not isinstance(choices, (list, tuple)) or not choices
            or not all(isinstance(c, str) and c for c in choices)):
        raise ValueError("guided_choice must be a non-empty list of non-empty strings")
    return "(" + "|".join(regex_escape(c) for c in choices) + ")"


# ---------------------------------------------------------------------------------------------
# JSON schema subset -> regex
# ---------------------------------------------------------------------------------------------
_WS = " ?"
# one character of a JSON string: printable ASCII but '"' and '\', an escape, or one well-formed
# multi-byte UTF-8 sequence (so every accepted text decodes)
_UTF8 = (r"[\xC2-\xDF][\x80-\xBF]|\xE0[\xA0-\xBF][\x80-\xBF]|[\xE1-\xEC\xEE\xEF][\x80-\xBF]{2}"
         r"|\xED[\x80-\x9F][\x80-\xBF]|\xF0[\x90-\xBF][\x80-\xBF]{2}"
         r"|[\xF1-\xF3][\x80-\xBF]{3}|\xF4[\x80-\x8F][\x80-\xBF]{2}")
_STR_CHAR = r'([\x20\x21\x23-\x5B\x5D-\x7E]|\\(["\\/bfnrt]|u[0-9a-fA-F]{4})|' + _UTF8 + ")"
_INT = r"-?(0|[1-9][0-9]*)"
_NUM = _INT + r"(\.[0-9]+)?([eE][+-]?[0-9]+)?"
_IGNORED = {"title", "description", "default", "examples", "$schema", "$id", "$comment",
            "$defs", "definitions", "additionalProperties", "deprecated", "readOnly",
            "writeOnly"}
_BY_TYPE = {
    "string": {"minLength", "maxLength", "pattern"},
    "array": {"items", "minItems", "maxItems"},
    "object": {"properties", "required"},
    "integer": set(), "number": set(), "boolean": set(), "null": set(),
}


def _const_regex(v) -> str:
    forms = {json.dumps(v, ensure_ascii=a, separators=s)
             for a in (True, False) for s in ((", ", ": "), (",", ":"))}
    alts = sorted(regex_escape(f) for f in forms)
    return alts[0] if len(alts) == 1 else "(" + "|".join(alts) + ")"


def schema_to_regex(schema) -> str:
    if isinstance(schema, str):
        try:
            schema = json.loads(schema)
        except json.JSONDecodeError as e:
            raise ValueError(f"guided_json is not valid JSON: {e}")
    if not isinstance(schema, dict):
        raise ValueError("a JSON schema must be an object")
    root = schema

    def resolve(ref: str):
        if not isinstance(ref, str) or not (ref == "#" or ref.startswith("#/")):
            raise ValueError(f"unsupported $ref {ref!r}: only local '#/...' references")
        node = root
        for part in ref[2:].split("/") if ref != "#" else ():
            part = part.replace("~1", "/").replace("~0", "~")
            if not isinstance(node, dict) or part not in node:
                raise ValueError(f"$ref {ref!r} does not resolve")
            node = node[part]
        return node

    def go(sc, stack: Tuple[str, ...]) -> str:
        if sc is True or sc == {}:
            raise ValueError("an unconstrained schema (any JSON value) needs free nesting, "
                             "which is not supported: give the value a type")
        if not isinstance(sc, dict):
            raise ValueError(f"unsupported schema {sc!r}")
        if "$ref" in sc:
            ref = sc["$ref"]
            if ref in stack:
                raise ValueError(f"recursive $ref {ref!r} is not supported")
            return go(resolve(ref), stack + (ref,))
        if "const" in sc:
            return _const_regex(sc["const"])
        if "enum" in sc:
            if not isinstance(sc["enum"], list) or not sc["enum"]:
                raise ValueError("enum must be a non-empty list")
            return "(" + "|".join(_const_regex(v) for v in sc["enum"]) + ")"
        for k in ("anyOf", "oneOf"):
            if k in sc:
                extra = set(sc) - _IGNORED - {k}
                if extra:
                    raise ValueError(f"unsupported schema keyword next to {k}: {sorted(extra)[0]}")
                if not isinstance(sc[k], list) or not sc[k]:
                    raise ValueError(f"{k} must be a non-empty list")
                return "(" + "|".join(go(x, stack) for x in sc[k]) + ")"
        ty = sc.get("type")
        if ty is None and "properties" in sc:
            ty = "object"
        if isinstance(ty, list):
            # each type with the keywords that speak about it
            known = set().union(*_BY_TYPE.values())
            for k in sc:
                if k not in _IGNORED and k != "type" and k not in known:
                    raise ValueError(f"unsupported schema keyword '{k}'")
            return "(" + "|".join(
                go({"type": t, **{k: v for k, v in sc.items() if k in _BY_TYPE.get(t, ())}},
                   stack) for t in ty) + ")"
        if ty not in _BY_TYPE:
            raise ValueError(f"unsupported or missing schema type {ty!r}")
        known = _BY_TYPE[ty]
        for k in sc:
            if k not in _IGNORED and k != "type" and k not in known:
                raise ValueError(f"unsupported schema keyword '{k}' for type {ty}")
        if ty == "string":
            if "pattern" in sc:
                pat = sc["pattern"]
                if not isinstance(pat, str):
                    raise ValueError("pattern must be a string")
                if pat.startswith("^"):
                    pat = pat[1:]
                if pat.endswith("$") and not _escaped_at(pat, len(pat) - 1):
                    pat = pat[:-1]
                return '"(' + pat + ')"'
            lo, hi = int(sc.get("minLength", 0)), sc.get("maxLength")
            if lo < 0 or (hi is not None and int(hi) < lo):
                raise ValueError("bad minLength / maxLength")
            q = "*" if (lo == 0 and hi is None) else "{%d,%s}" % (lo, "" if hi is None else int(hi))
            return '"' + _STR_CHAR + q + '"'
        if ty == "integer":
            return _INT
        if ty == "number":
            return _NUM
        if ty == "boolean":
            return "(true|false)"
        if ty == "null":
            return "null"
        if ty == "array":
            if "items" not in sc:
                raise ValueError("an array schema needs 'items'")
            item = go(sc["items"], stack)
            lo, hi = int(sc.get("minItems", 0)), sc.get("maxItems")
            hi = None if hi is None else int(hi)
            if lo < 0 or (hi is not None and hi < lo):
                raise ValueError("bad minItems / maxItems")
            if hi == 0:
                return r"\[\]"
            more = "(," + _WS + item + "){%d,%s}" % (max(lo - 1, 0), "" if hi is None else hi - 1)
            body = "(" + item + more + ")"
            return r"\[" + (body if lo > 0 else body + "?") + r"\]"
        # object: properties in declaration order, the optional ones may be left out
        props = sc.get("properties", {})
        if not isinstance(props, dict):
            raise ValueError("properties must be an object")
        req = sc.get("required", [])
        unknown = [r for r in req if r not in props]
        if unknown:
            raise ValueError(f"required property '{unknown[0]}' has no schema in properties")
        mem = [(regex_escape(json.dumps(k)) + ":" + _WS + go(v, stack), k in req)
               for k, v in props.items()]

        def rest(i: int, first: bool) -> str:
            if i == len(mem):
                return ""
            m, required = mem[i]
            if not first:
                body = "," + _WS + m
                return (body if required else "(" + body + ")?") + rest(i + 1, False)
            taken = m + rest(i + 1, False)
            if required:
                return taken
            return "(" + taken + "|" + rest(i + 1, True) + ")"

        return r"\{" + rest(0, True) + r"\}"

    return go(schema, ("#",))


# ---------------------------------------------------------------------------------------------
# request fields -> grammar
# ---------------------------------------------------------------------------------------------
KINDS = ("regex", "choice", "json")


@dataclass
class Grammar:
    kind: str
    payload: str                 # canonical text of the request field
    trans: np.ndarray            # int32 [S, 256], -1 = dead
    accept: np.ndarray           # bool [S]
    compile_seconds: float = 0.0

    @property
    def num_states(self) -> int:
        return int(self.trans.shape[0])

    @property
    def digest(self) -> str:
        return guided_digest(self.kind, self.payload)

    def matches(self, data: bytes) -> bool:
        return dfa_matches(self.trans, self.accept, data)

    def walk(self, data: bytes, state: int = 0) -> int:
        for b in data:
            if state < 0:
                break
            state = int(self.trans[state, b])
        return state


def guided_digest(kind: str, payload: str) -> str:
    return hashlib.sha256((kind + "\0" + payload).encode("utf-8")).hexdigest()


def canonical(kind: str, value) -> str:
    if kind not in KINDS:
        raise ValueError(f"unknown guided decoding kind {kind!r}")
    if kind == "regex":
        if not isinstance(value, str) or not value:
            raise ValueError("guided_regex must be a non-empty string")
        return value
    if kind == "choice":
        choice_to_regex(value)
        return json.dumps(list(value), ensure_ascii=False)
    if isinstance(value, str):
        try:
            value = json.loads(value)
        except json.JSONDecodeError as e:
            raise ValueError(f"guided_json is not valid JSON: {e}")
    if not isinstance(value, dict):
        raise ValueError("guided_json must be a JSON schema object")
    return json.dumps(value, ensure_ascii=False)   # key order kept: it is the emission order


def guided_regex_of(kind: str, payload: str) -> str:
    if kind == "regex":
        return payload
    if kind == "choice":
        return choice_to_regex(json.loads(payload))
    return schema_to_regex(json.loads(payload))


_grammars: "OrderedDict[Tuple[str, int], Grammar]" = OrderedDict()


def compile_guided(kind: str, payload: str, max_states: int = 4096) -> Grammar:
    """The byte DFA of a (kind, canonical payload); a small per-process LRU keeps repeats of one
    schema from compiling again."""
    key = (guided_digest(kind, payload), int(max_states))
    g = _grammars.get(key)
    if g is not None:
        _grammars.move_to_end(key)
        return g
    t0 = time.perf_counter()
    trans, accept = compile_regex(guided_regex_of(kind, payload), max_states)
    g = Grammar(kind, payload, trans, accept, time.perf_counter() - t0)
    _grammars[key] = g
    while len(_grammars) > 64:
        _grammars.popitem(last=False)
    return g


def parse_guided_fields(body: dict) -> Optional[Tuple[str, str]]:
    """The (kind, canonical payload) of an OpenAI / vLLM request body, or None.  ``ValueError``
    for more than one guided field, ``json_object`` and malformed fields."""
    found = []
    for name, kind in (("guided_regex", "regex"), ("guided_choice", "choice"),
                       ("guided_json", "json")):
        if body.get(name) is not None:
            found.append((kind, body[name]))
    rf = body.get("response_format")
    if rf is not None:
        if not isinstance(rf, dict) or "type" not in rf:
            raise ValueError("response_format must be an object with a 'type'")
        t = rf["type"]
        if t == "json_object":
            raise ValueError("response_format 'json_object' is not supported (free nesting needs "
                             "more than a finite automaton): send a schema with "
                             "{'type': 'json_schema', 'json_schema': {'schema': ...}}")
        if t == "json_schema":
            js = rf.get("json_schema")
            if not isinstance(js, dict) or not isinstance(js.get("schema"), (dict, str)):
                raise ValueError("response_format json_schema needs json_schema.schema")
            found.append(("json", js["schema"]))
        elif t != "text":
            raise ValueError(f"unknown response_format type {t!r}")
    if not found:
        return None
    if len(found) > 1:
        raise ValueError("only one of guided_regex, guided_choice, guided_json and "
                         "response_format json_schema may be given")
    kind, value = found[0]
    return kind, canonical(kind, value)


# ---------------------------------------------------------------------------------------------
# tokenizer -> bytes of every token
# ---------------------------------------------------------------------------------------------
def _gpt2_unicode_to_byte() -> Dict[str, int]:
    bs = (list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1))
          + list(range(0xAE, 0xFF + 1)))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {chr(c): b for b, c in zip(bs, cs)}


_BYTE_TOKEN = _re.compile(r"^<0x([0-9A-Fa-f]{2})>$")


def token_bytes(tokenizer) -> List[Optional[bytes]]:
    """The byte string every token id stands for; None for special / added tokens and ids
    without text."""
    from ..data.tokenizer import ByteTokenizer

    if isinstance(tokenizer, ByteTokenizer):
        out: List[Optional[bytes]] = [None] * tokenizer.vocab_size
        for b in range(256):
            if tokenizer.offset + b < tokenizer.vocab_size:
                out[tokenizer.offset + b] = bytes([b])
        return out
    tok = getattr(tokenizer, "tok", tokenizer)
    if not hasattr(tok, "get_vocab"):
        raise ValueError(f"guided decoding does not know the tokenizer {type(tokenizer).__name__}")
    vocab = tok.get_vocab(with_added_tokens=True)
    added = set(tok.get_added_tokens_decoder().keys())
    spec = json.loads(tok.to_str())
    byte_level = "ByteLevel" in json.dumps([spec.get("pre_tokenizer"), spec.get("decoder")])
    out = [None] * (max(vocab.values()) + 1 if vocab else 0)
    u2b = _gpt2_unicode_to_byte() if byte_level else None
    for text, i in vocab.items():
        if i in added or not text:
            continue
        if byte_level:
            try:
                out[i] = bytes(u2b[c] for c in text)
            except KeyError:
                out[i] = None
            continue
        m = _BYTE_TOKEN.match(text)
        out[i] = bytes([int(m.group(1), 16)]) if m else text.replace("▁", " ").encode("utf-8")
    return out


def tokenizer_identity(tokenizer) -> str:
    from ..data.tokenizer import ByteTokenizer

    if isinstance(tokenizer, ByteTokenizer):
        return f"byte:{tokenizer.vocab_size}"
    path = getattr(tokenizer, "path", None)
    return f"hf:{path}" if path else f"obj:{id(tokenizer)}"


# ---------------------------------------------------------------------------------------------
# token index
# ---------------------------------------------------------------------------------------------
def build_token_index(trans: np.ndarray, accept: np.ndarray, tok_bytes: List[Optional[bytes]],
                      vocab: int, eos_id: Optional[int], device="cpu"):
    """(next int16 [S, vocab] on ``device``, live bool [S] numpy).  One gather per byte position
    over [states chunk, V]; then states that are not accepting and allow no token are dropped
    (their incoming entries become -1) until none is left."""
    S = int(trans.shape[0])
    if S > 32767:
        raise ValueError("a token table holds at most 32767 states")
    dev = torch.device(device)
    n_tok = min(len(tok_bytes), vocab)
    lens = np.zeros(vocab, dtype=np.int64)
    for t in range(n_tok):
        if tok_bytes[t]:
            lens[t] = len(tok_bytes[t])
    Lmax = int(lens.max()) if vocab else 0
    pad = np.zeros((vocab, max(Lmax, 1)), dtype=np.int64)
    for t in np.nonzero(lens)[0]:
        pad[t, :lens[t]] = np.frombuffer(tok_bytes[t], dtype=np.uint8)
    tb = torch.from_numpy(pad).to(dev)
    ln = torch.from_numpy(lens).to(dev)
    tr = torch.from_numpy(np.asarray(trans)).to(dev).long()
    tr = torch.where(tr < 0, torch.full_like(tr, S), tr)
    tr = torch.cat([tr, torch.full((1, 256), S, dtype=torch.long, device=dev)])   # row S: dead
    nxt = torch.empty(S, vocab, dtype=torch.int16, device=dev)
    chunk = max(1, (4 << 20) // max(vocab, 1))
    for s0 in range(0, S, chunk):
        s1 = min(S, s0 + chunk)
        cur = torch.arange(s0, s1, device=dev)[:, None].expand(s1 - s0, vocab)
        for pos in range(Lmax):
            step = tr[cur, tb[:, pos][None, :]]
            cur = torch.where((pos < ln)[None, :], step, cur)
        cur = torch.where((cur == S) | (ln == 0)[None, :], torch.full_like(cur, -1), cur)
        nxt[s0:s1] = cur.to(torch.int16)
    acc = torch.from_numpy(np.asarray(accept, dtype=bool)).to(dev)
    if eos_id is not None and 0 <= eos_id < vocab:
        ar = torch.arange(S, device=dev, dtype=torch.int16)
        nxt[:, eos_id] = torch.where(acc, ar, torch.full_like(ar, -1))
    live = torch.ones(S + 1, dtype=torch.bool, device=dev)
    live[S] = False
    eos_col = eos_id if eos_id is not None and 0 <= eos_id < vocab else None
    while True:
        idx = nxt.long()
        idx = torch.where(idx < 0, torch.full_like(idx, S), idx)
        ok = live[idx]
        if eos_col is not None:
            ok[:, eos_col] = False          # EOS is not a way forward
        new = live.clone()
        new[:S] = live[:S] & (acc | ok.any(dim=1))
        dead_target = (nxt >= 0) & ~new[idx]
        if eos_col is not None:
            dead_target[:, eos_col] = False
        if bool((new == live).all()) and not bool(dead_target.any()):
            break
        nxt[dead_target] = -1
        live = new
    if not bool(live[0]):
        raise ValueError("the tokenizer's vocabulary cannot spell any text the grammar accepts")
    return nxt, live[:S].cpu().numpy()


@dataclass
class TokenTable:
    grammar: Grammar
    next: torch.Tensor           # int16 [S, V] on the engine's device
    live: np.ndarray
    refs: int = 0                # running sequences that hold it

    @property
    def nbytes(self) -> int:
        return self.next.numel() * 2

    @property
    def address(self) -> int:
        return self.next.data_ptr()


class GuidedCache:
    """Token tables by (grammar digest, tokenizer identity): LRU, bounded in bytes; a table a
    running sequence holds is never evicted."""

    def __init__(self, max_bytes: int):
        self.max_bytes = int(max_bytes)
        self.tables: "OrderedDict[str, TokenTable]" = OrderedDict()
        self.hits = 0
        self.misses = 0
        self.compile_seconds = 0.0

    @property
    def nbytes(self) -> int:
        return sum(t.nbytes for t in self.tables.values())

    def get(self, key: str, build) -> TokenTable:
        t = self.tables.get(key)
        if t is not None:
            self.hits += 1
            self.tables.move_to_end(key)
            return t
        self.misses += 1
        t0 = time.perf_counter()
        t = build()
        self.compile_seconds += time.perf_counter() - t0
        self.tables[key] = t
        self.evict(keep=key)
        return t

    def evict(self, keep: Optional[str] = None) -> None:
        total = self.nbytes
        for k in list(self.tables):
            if total <= self.max_bytes:
                break
            t = self.tables[k]
            if t.refs > 0 or k == keep:
                continue
            total -= t.nbytes
            del self.tables[k]
