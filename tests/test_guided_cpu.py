"""Guided decoding on the host: the regex compiler against ``re``, the token index against a
byte-by-byte walk, token bytes of three tokenizer kinds, JSON schemas against ``json``, the
request fields through the API, and the CPU engine end to end."""
import itertools
import json
import random
import re

import numpy as np
import pytest
import torch

from lumen.data.tokenizer import ByteTokenizer
from lumen.serve import guided as G
from lumen.serve.sequence import SamplingParams

# ---- regex vs re ----------------------------------------------------------------------------------
# (pattern, 5-symbol alphabet): every string up to length 6 over the alphabet is tried
PATTERNS = [
    (r"(yes|no), [0-9]{3}\.", "y0, ."), (r"(yes|no)", "yesno"), (r"[0-9]{3}\.", "019.a"),
    (r"[^a]b*", "ab\nc "), (r"(ab|a)(c|bc)?", "abcd "), (r"\d{1,3}(\.\d{1,3}){3}", "12.a9"),
    (r"a.c", "abc\nd"), (r"a*?b+?c??", "abcd "), (r"(?:ab)+|c{2,}", "abcx "),
    (r"\w+\s\W", "a_ -1"), (r"[a-c\d]*x", "abc1x"), (r"^ab$", "abc$^"), (r"[\]a-]+", "]a-bc"),
    (r"a{2}b{0,2}", "ab{},"), (r"\\\.\(\)", "\\.()a"), (r"\D\S\W", "a1 _-"),
    (r"(a|b|)c", "abc| "), (r"[^\d\s]+\t?\n", "a1 \t\n"), (r"(a(b(c)?)*)+", "abcd "),
    (r"x{2,}?y{1,2}?", "xyz{,"), (r"[.*+?]{2}", ".*+?a"),
]


@pytest.mark.parametrize("pattern,alphabet", PATTERNS)
def test_regex_dfa_equals_re_fullmatch(pattern, alphabet):
    assert len(set(alphabet)) == 5
    trans, accept = G.compile_regex(pattern)
    assert trans.dtype == np.int32 and trans.shape[1] == 256 and accept.shape == (len(trans),)
    # trimmed: every state reaches an accepting one (so a constrained sequence can finish)
    good = accept.copy()
    for _ in range(len(trans)):
        good |= np.where(trans >= 0, good[np.maximum(trans, 0)], False).any(axis=1)
    assert good.all()
    rx = re.compile(pattern)
    n = 0
    for L in range(7):
        for t in itertools.product(alphabet, repeat=L):
            s = "".join(t)
            assert G.dfa_matches(trans, accept, s.encode()) == (rx.fullmatch(s) is not None), s
            n += 1
    assert n == 19531


def test_regex_non_ascii_literals_are_utf8():
    trans, accept = G.compile_regex("(é|ü)+x[äö]")
    assert G.dfa_matches(trans, accept, "éüéxö".encode())
    assert not G.dfa_matches(trans, accept, "éx".encode())
    assert not G.dfa_matches(trans, accept, "é".encode()[:1] + b"x\xc3\xa4")
    t2, a2 = G.compile_regex("[^a]")        # a negated class takes any other single byte
    assert G.dfa_matches(t2, a2, b"\xff") and not G.dfa_matches(t2, a2, b"a")


@pytest.mark.parametrize("pattern,what", [
    (r"(a)\1", "backreference"), (r"(?P=n)", "backreference"), (r"(?=a)b", "lookaround"),
    (r"(?<!a)b", "lookaround"), (r"(?P<n>a)", "named group"), (r"(?i)a", "inline flags"),
    (r"a^b", "anchor"), (r"a$b", "anchor"), (r"a\b", "anchor"), (r"a**", "quantifier"),
    (r"(a", "unbalanced"), (r"a)", "unbalanced"), (r"[a", "unbalanced"), (r"a{3,1}", "repeat"),
])
def test_regex_unsupported_constructs_raise(pattern, what):
    with pytest.raises(ValueError, match=what):
        G.compile_regex(pattern)


def test_state_cap_and_empty_language():
    with pytest.raises(ValueError, match="states"):
        G.compile_regex(r"[ab]*a[ab]{12}", max_states=256)     # 2^13 states
    with pytest.raises(ValueError, match="nothing"):
        G.compile_regex(r"a[^\x00-\xff]")


def test_choice_is_alternation_of_escaped_literals():
    g = G.compile_guided("choice", G.canonical("choice", ["a.b", "(x)", "yes", "yeah"]))
    for s in ("a.b", "(x)", "yes", "yeah"):
        assert g.matches(s.encode())
    for s in ("axb", "x", "ye", "yesyeah", ""):
        assert not g.matches(s.encode())
    with pytest.raises(ValueError):
        G.canonical("choice", [])


# ---- token index vs brute force -----------------------------------------------------------------
def _vocab():
    """~300 tokens: 3 specials, the 256 bytes, multi-byte and overlapping tokens; the model's V
    (320) is padded past the tokenizer's vocabulary."""
    multi = [b"ab", b"abe", b"abee", b"be", b"ee", b"e", b"cd", b"cde", b"dee", b"ye", b"yes",
             b"yeah", b"ah", b"no", b"n", b"o", "é".encode(), "éé".encode(), b"12", b"123", b"1.",
             b".1", b"..", b"{\"", b"\":", b"\": ", b", \"", b"true", b"false", b"tr", b"ue",
             b"}", b"\"}", b"a" * 5, b"0", b"00", b"000", b" ", b"  ", b"\n", b"a\n"]
    tb = [None, None, None] + [bytes([b]) for b in range(256)] + multi
    return tb, 320, 2


def _walk(trans, s, data):
    for b in data:
        if s < 0:
            return -1
        s = int(trans[s, b])
    return s


@pytest.mark.parametrize("pattern", [r"(ab|cd)e{2}", r"(yes|yeah|no)", r"\d{1,3}(\.\d{1,3}){3}",
                                     r"é+a{5}", r'\{"k": ?(true|false)\}', r"[^a]b*\n?"])
def test_token_index_equals_byte_walk(pattern):
    tb, V, eos = _vocab()
    assert 290 <= len(tb) <= 310
    trans, accept = G.compile_regex(pattern)
    nxt, live = G.build_token_index(trans, accept, tb, V, eos)
    assert nxt.dtype == torch.int16 and tuple(nxt.shape) == (len(trans), V) and live.all()
    nx = nxt.numpy()
    for s in range(len(trans)):
        for t in range(V):
            if t == eos:
                want = s if accept[s] else -1          # EOS exactly in accepting states
            elif t >= len(tb) or tb[t] is None:
                want = -1                              # no bytes / past the tokenizer's vocabulary
            else:
                want = _walk(trans, s, tb[t])
            assert nx[s, t] == want, (s, t)
        if not accept[s]:
            assert (np.delete(nx[s], eos) >= 0).any()  # a live state can always go on


def test_token_index_prunes_states_the_vocabulary_cannot_leave():
    tb = [None, None, None] + [bytes([b]) for b in b"abc"] + [b"ab"]
    trans, accept = G.compile_regex(r"(ab|cd)e?")
    nxt, live = G.build_token_index(trans, accept, tb, 8, 2)
    nx = nxt.numpy()
    after_c = int(trans[0, ord("c")])
    assert after_c >= 0 and not live[after_c] and nx[0, 5] == -1       # 'c' leads nowhere
    assert nx[0, 3] >= 0 and nx[0, 6] >= 0                             # 'a' and 'ab' stay
    for s in np.nonzero(live)[0]:
        ok = [t for t in range(8) if t != 2 and nx[s, t] >= 0]
        assert accept[s] or ok
        assert all(live[nx[s, t]] for t in ok)
    with pytest.raises(ValueError, match="vocabulary"):
        G.build_token_index(*G.compile_regex(r"d+"), tb, 8, 2)


# ---- token bytes ------------------------------------------------------------------------------------
def test_token_bytes_byte_tokenizer():
    tb = G.token_bytes(ByteTokenizer(512))
    assert len(tb) == 512 and tb[:3] == [None] * 3 and all(t is None for t in tb[259:])
    assert [tb[3 + b] for b in range(256)] == [bytes([b]) for b in range(256)]


def test_token_bytes_sentencepiece_style():
    from tokenizers import Tokenizer, decoders, models

    vocab = {"<unk>": 0, "<s>": 1, "</s>": 2}
    for b in range(256):
        vocab["<0x%02X>" % b] = 3 + b
    words = ["▁hello", "▁", "é", "lo", "▁wor▁ld"]
    for t in words:
        vocab[t] = len(vocab)
    tk = Tokenizer(models.BPE(vocab=vocab, merges=[], unk_token="<unk>", byte_fallback=True))
    tk.add_special_tokens(["<unk>", "<s>", "</s>"])
    tk.decoder = decoders.Sequence([decoders.Replace("▁", " "), decoders.ByteFallback(),
                                    decoders.Fuse()])
    tb = G.token_bytes(tk)
    assert tb[:3] == [None] * 3
    assert [tb[3 + b] for b in range(256)] == [bytes([b]) for b in range(256)]
    assert tb[259:] == [b" hello", b" ", "é".encode(), b"lo", b" wor ld"]


def test_token_bytes_byte_level_bpe():
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers

    b2u = {b: u for u, b in G._gpt2_unicode_to_byte().items()}
    assert len(b2u) == 256 and b2u[0x20] == "Ġ" and b2u[0x41] == "A"
    vocab = {b2u[b]: b for b in range(256)}
    extra = [b" hello", b"he", "é".encode(), b"\n\n"]
    for t in extra:
        vocab["".join(b2u[x] for x in t)] = len(vocab)
    vocab["<|endoftext|>"] = len(vocab)
    tk = Tokenizer(models.BPE(vocab=vocab, merges=[]))
    tk.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tk.decoder = decoders.ByteLevel()
    tk.add_special_tokens(["<|endoftext|>"])
    tb = G.token_bytes(tk)
    assert [tb[b] for b in range(256)] == [bytes([b]) for b in range(256)]
    assert tb[256:] == extra + [None]


# ---- JSON schema ------------------------------------------------------------------------------------
FLAT = {"type": "object",
        "properties": {"ok": {"type": "boolean"}, "color": {"enum": ["red", "green", 3, None]},
                       "id": {"type": "string", "pattern": "^[a-z]{2}-[0-9]{1,2}$"},
                       "note": {"type": "string", "maxLength": 4}},
        "required": ["ok", "id"]}
NESTED = {"type": "object",
          "properties": {"name": {"type": "string", "minLength": 1, "maxLength": 6},
                         "args": {"type": "object",
                                  "properties": {"n": {"type": "integer"},
                                                 "x": {"type": "number"},
                                                 "z": {"type": "null"}},
                                  "required": ["n"]}},
          "required": ["name", "args"]}
ARRAY = {"type": "array", "items": {"$ref": "#/$defs/item"}, "minItems": 1, "maxItems": 3,
         "$defs": {"item": {"type": "integer"}}}
ANYOF = {"anyOf": [{"type": "boolean"}, {"const": "n/a"},
                   {"type": "array", "items": {"oneOf": [{"type": "null"}, {"type": "string",
                                                                            "maxLength": 2}]},
                    "maxItems": 2}]}


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _check_flat(v):
    return (isinstance(v, dict) and set(v) <= {"ok", "color", "id", "note"}
            and isinstance(v.get("ok"), bool) and isinstance(v.get("id"), str)
            and re.fullmatch(r"[a-z]{2}-[0-9]{1,2}", v["id"]) is not None
            and ("color" not in v or v["color"] in ("red", "green", None)
                 or (_is_int(v["color"]) and v["color"] == 3))
            and ("note" not in v or (isinstance(v["note"], str) and len(v["note"]) <= 4))
            and list(v) == [k for k in ("ok", "color", "id", "note") if k in v])


def _check_nested(v):
    if not (isinstance(v, dict) and list(v) == ["name", "args"]):
        return False
    a = v["args"]
    return (isinstance(v["name"], str) and 1 <= len(v["name"]) <= 6 and isinstance(a, dict)
            and set(a) <= {"n", "x", "z"} and _is_int(a.get("n"))
            and ("x" not in a or (isinstance(a["x"], (int, float)) and not isinstance(a["x"], bool)))
            and ("z" not in a or a["z"] is None))


def _check_array(v):
    return isinstance(v, list) and 1 <= len(v) <= 3 and all(_is_int(x) for x in v)


def _check_anyof(v):
    if isinstance(v, bool) or v == "n/a":
        return True
    return (isinstance(v, list) and len(v) <= 2
            and all(x is None or (isinstance(x, str) and len(x) <= 2) for x in v))


SCHEMAS = {
    "flat": (FLAT, _check_flat,
             [{"ok": True, "id": "ab-1"}, {"ok": False, "color": "red", "id": "zz-42"},
              {"ok": True, "color": 3, "id": "qq-0", "note": "é\"\\"},
              {"ok": False, "color": None, "id": "ab-12", "note": ""}],
             [{"ok": True}, {"id": "ab-1", "ok": True}, {"ok": 1, "id": "ab-1"},
              {"ok": True, "id": "abc-1"}, {"ok": True, "id": "ab-1", "note": "12345"},
              {"ok": True, "color": "blue", "id": "ab-1"}, {"ok": True, "id": "ab-1", "more": 1}]),
    "nested": (NESTED, _check_nested,
               [{"name": "f", "args": {"n": 0}}, {"name": "search", "args": {"n": -12, "x": 1.5}},
                {"name": "ü", "args": {"n": 7, "x": 2e3, "z": None}},
                {"name": "g", "args": {"n": 3, "z": None}}],
               [{"name": "", "args": {"n": 0}}, {"name": "f", "args": {}},
                {"name": "f", "args": {"n": 1.5}}, {"name": "toolong", "args": {"n": 1}},
                {"args": {"n": 0}, "name": "f"}, {"name": "f", "args": {"n": 1, "z": 0}},
                {"name": "f"}]),
    "array": (ARRAY, _check_array, [[1], [1, -2], [0, 10, 999]],
              [[], [1, 2, 3, 4], [1.5], ["1"], [True], 1]),
    "anyof": (ANYOF, _check_anyof, [True, False, "n/a", [], [None], ["ab", None], ["", "é"]],
              [None, "n/b", [None, None, None], ["abc"], [1], 0]),
}


def _distances(trans, accept):
    """Fewest bytes from every state to an accepting one."""
    S = len(trans)
    d = np.where(accept, 0, S + 1)
    for _ in range(S):
        t = np.where(trans >= 0, d[np.maximum(trans, 0)], S + 1).min(axis=1) + 1
        d = np.minimum(d, t)
    return d


@pytest.mark.parametrize("name", list(SCHEMAS))
def test_json_schema_accepts_rejects_and_generates(name):
    schema, check, valid, invalid = SCHEMAS[name]
    g = G.compile_guided("json", G.canonical("json", schema))
    print(f"schema {name}: {g.num_states} states, compiled in {g.compile_seconds * 1e3:.1f} ms")
    for v in valid:
        assert check(v), v
        for sep in ((", ", ": "), (",", ":")):
            assert g.matches(json.dumps(v, separators=sep).encode()), (v, sep)
        assert g.matches(json.dumps(v, ensure_ascii=False).encode()), v
    for v in invalid:
        assert not check(v), v
        for sep in ((", ", ": "), (",", ":")):
            assert not g.matches(json.dumps(v, separators=sep).encode()), (v, sep)
    nested = next(v for v in valid if isinstance(v, (dict, list)) and v)
    assert not g.matches(json.dumps(nested, indent=1).encode())       # no newlines
    # random walks through the automaton: whatever it accepts parses and satisfies the schema
    rng = random.Random(0)
    d = _distances(g.trans, g.accept)
    for _ in range(200):
        s, out = 0, bytearray()
        while True:
            if g.accept[s] and (len(out) > 40 or rng.random() < 0.3 or (g.trans[s] < 0).all()):
                break
            nb = [b for b in range(256) if g.trans[s, b] >= 0]
            if len(out) > 40 or rng.random() < 0.3:              # head for the exit
                nb = [b for b in nb if d[g.trans[s, b]] < d[s]] or nb
            b = rng.choice(nb)
            out.append(b)
            s = int(g.trans[s, b])
        v = json.loads(bytes(out))
        assert check(v), bytes(out)


def test_json_schema_type_list_keeps_each_types_keywords():
    g = G.compile_guided("json", G.canonical("json", {"type": ["string", "null"], "maxLength": 3}))
    assert g.matches(b"null") and g.matches(b'"abc"')
    assert not g.matches(b'"abcd"') and not g.matches(b"1")
    with pytest.raises(ValueError, match="minimum"):
        G.schema_to_regex({"type": ["integer", "null"], "minimum": 1})


def test_json_schema_rejections():
    rec = {"type": "object", "properties": {"next": {"$ref": "#"}}}
    with pytest.raises(ValueError, match="recursive"):
        G.schema_to_regex(rec)
    rec2 = {"$ref": "#/$defs/a", "$defs": {"a": {"type": "array", "items": {"$ref": "#/$defs/a"}}}}
    with pytest.raises(ValueError, match="recursive"):
        G.schema_to_regex(rec2)
    for bad in ({"type": "integer", "minimum": 3}, {"type": "string", "format": "date"},
                {"type": "object", "patternProperties": {"a": {}}}, {"type": "array"},
                {"not": {"type": "null"}}, {}, {"type": "tuple"}):
        with pytest.raises(ValueError):
            G.schema_to_regex(bad)


# ---- request fields ---------------------------------------------------------------------------------
def test_sampling_params_guided_validation():
    p = SamplingParams(guided={"regex": "a+"})
    assert p.guided == ("regex", "a+") and p.row_features
    assert SamplingParams(guided=("choice", '["a", "b"]')).guided[0] == "choice"
    assert SamplingParams(**vars(p)).guided == p.guided
    with pytest.raises(ValueError, match="one"):
        SamplingParams(guided={"regex": "a+", "choice": ["a"]})
    with pytest.raises(ValueError, match="min_tokens"):
        SamplingParams(guided={"regex": "a+"}, min_tokens=2)
    assert not SamplingParams().row_features


def test_parse_guided_fields():
    assert G.parse_guided_fields({"prompt": "x"}) is None
    assert G.parse_guided_fields({"response_format": {"type": "text"}}) is None
    assert G.parse_guided_fields({"guided_regex": "a|b"}) == ("regex", "a|b")
    assert G.parse_guided_fields({"guided_choice": ["a", "b"]}) == ("choice", '["a", "b"]')
    sc = {"type": "boolean"}
    want = ("json", json.dumps(sc))
    assert G.parse_guided_fields({"guided_json": sc}) == want
    assert G.parse_guided_fields({"guided_json": json.dumps(sc)}) == want
    rf = {"type": "json_schema", "json_schema": {"name": "b", "schema": sc}}
    assert G.parse_guided_fields({"response_format": rf}) == want
    with pytest.raises(ValueError, match="json_schema"):
        G.parse_guided_fields({"response_format": {"type": "json_object"}})
    with pytest.raises(ValueError, match="only one"):
        G.parse_guided_fields({"guided_regex": "a", "response_format": rf})


@pytest.fixture(scope="module")
def model():
    from lumen.models import build_model

    torch.manual_seed(0)
    m = build_model("tiny-llama-gqa", dtype=torch.float32, device="cpu", init="random", seed=1)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 2:
                p.mul_(5.0)
    return m.eval()


def _engine(model, **kw):
    from lumen.serve.engine import EngineConfig, LLMEngine

    kw.setdefault("num_blocks", 128)
    return LLMEngine(EngineConfig(model="tiny-llama-gqa", device="cpu", max_model_len=256,
                                  block_size=4, use_graphs=False, **kw), model=model,
                     tokenizer=ByteTokenizer(512))


def _api_checks(c, params_seen):
    base = {"prompt": "hi", "max_tokens": 12, "temperature": 0}
    r = c.post("/v1/completions", json=dict(base, guided_regex=r"(ab|cd)e{2}"))
    assert r.status_code == 200 and r.json()["choices"][0]["text"] in ("abee", "cdee")
    assert r.json()["choices"][0]["finish_reason"] == "stop"
    r = c.post("/v1/completions", json=dict(base, guided_choice=["yes", "yeah", "no"]))
    assert r.json()["choices"][0]["text"] in ("yes", "yeah", "no")
    sc = {"type": "object", "properties": {"ok": {"type": "boolean"}}, "required": ["ok"]}
    r = c.post("/v1/completions", json=dict(base, max_tokens=20, guided_json=sc))
    assert set(json.loads(r.json()["choices"][0]["text"])) == {"ok"}
    rf = {"type": "json_schema", "json_schema": {"name": "x", "schema": sc}}
    chat = {"messages": [{"role": "user", "content": "hi"}], "max_tokens": 20, "temperature": 0}
    r = c.post("/v1/chat/completions", json=dict(chat, response_format=rf))
    assert isinstance(json.loads(r.json()["choices"][0]["message"]["content"])["ok"], bool)
    r = c.post("/v1/chat/completions", json=dict(chat, response_format={"type": "text"}))
    assert r.status_code == 200
    assert [p.guided[0] if p.guided else None for p in params_seen] == [
        "regex", "choice", "json", "json", None]
    bad = [dict(base, guided_regex="a", guided_choice=["a"]), dict(base, guided_regex=r"(a)\1"),
           dict(base, response_format={"type": "json_object"}),
           dict(base, guided_regex="a+", min_tokens=2),
           dict(base, guided_regex=r"[ab]*a[ab]{12}"),
           dict(base, guided_json={"type": "object", "properties": {"a": {"$ref": "#"}}})]
    for body in bad:
        r = c.post("/v1/completions", json=body)
        assert r.status_code == 400, body
    assert "json_schema" in c.post("/v1/completions", json=bad[2]).json()["detail"]
    assert len(params_seen) == 5                     # nothing rejected reached the engine
    m = c.get("/metrics").text
    assert "lumen_guided_requests_total 4" in m and "lumen_guided_cache_hits_total" in m
    assert "lumen_guided_compile_seconds_total" in m


def test_api_guided_fields_in_process(model):
    from starlette.testclient import TestClient

    from lumen.serve.api_server import create_app
    from lumen.serve.engine import AsyncEngine

    eng = _engine(model, guided_max_states=256)
    seen = []
    add = eng.add_request

    def spy(prompt, params=None, *a, **kw):
        seen.append(params)
        return add(prompt, params, *a, **kw)
    eng.add_request = spy
    ae = AsyncEngine(eng)
    try:
        _api_checks(TestClient(create_app(ae, "tiny")), seen)
    finally:
        ae.shutdown()
    assert eng.blocks.num_free == eng.blocks.num_blocks


def test_api_guided_fields_through_engine_core(model):
    """The same with the engine core behind the process protocol: the API side ships the
    compiled automaton, the core builds and caches the token table."""
    import queue
    import threading

    from starlette.testclient import TestClient

    from lumen.serve.api_server import create_app
    from lumen.serve.frontend import EngineCoreClient, run_engine_core

    eng = _engine(model, guided_max_states=256)
    seen = []
    add = eng.add_request

    def spy(prompt, params=None, *a, **kw):
        assert params.guided is None or params.guided_dfa is not None
        seen.append(params)
        return add(prompt, params, *a, **kw)
    eng.add_request = spy
    req_q, out_q = queue.Queue(), queue.Queue()
    core = threading.Thread(target=run_engine_core, args=(eng, req_q, [out_q]), daemon=True)
    core.start()
    client = EngineCoreClient(req_q, out_q, eng.tokenizer, "tiny", 256, eng.eos_id,
                              guided_max_states=256)
    try:
        _api_checks(TestClient(create_app(client, "tiny")), seen)
    finally:
        req_q.put(("stop",))
        core.join(timeout=30)
        out_q.put(None)
    assert eng.guided_stats()["guided_cache_hits"] >= 1      # the one schema, asked twice


# ---- CPU engine end to end --------------------------------------------------------------------------
@pytest.mark.parametrize("async_sched", [True, False])
def test_cpu_engine_guided_end_to_end(model, async_sched):
    """Finite languages only: the grammar, not the random weights, guarantees termination."""
    eng = _engine(model, async_scheduling=async_sched, max_num_seqs=4)
    reqs = [("regex", r"(ab|cd)e{2}", 0.0, None), ("choice", ["yes", "yeah", "no"], 1.0, 5),
            (None, None, 1.0, 7), ("regex", r"[0-9]{3}-[a-c]{2}", 1.0, 9), (None, None, 0.0, None),
            ("choice", ["yes", "yeah", "no"], 0.0, None), ("regex", r"x{2,9}", 1.0, 3)]
    seqs = []
    for i, (kind, val, T, seed) in enumerate(reqs):
        sp = SamplingParams(max_tokens=16, temperature=T, seed=seed,
                            guided=None if kind is None else {kind: val},
                            ignore_eos=kind is None)
        seqs.append(eng.add_request([5 + i, 9, 33, 7], sp))
    while eng.has_work:
        eng.step()
    for (kind, val, _, _), s in zip(reqs, seqs):
        if kind is None:
            assert len(s.output_ids) == 16
            continue
        assert s.finish_reason == "stop" and s.output_ids[-1] == eng.eos_id
        text = eng.tokenizer.decode(s.output_ids[:-1])
        assert G.compile_guided(kind, G.canonical(kind, val)).matches(text.encode()), text
    assert eng.guided_state.num_free == 4 and all(s.guided_slot == -1 for s in seqs)
    assert all(t.refs == 0 for t in eng.guided_cache.tables.values())
    assert eng.blocks.num_free == eng.blocks.num_blocks
    # the seeded unguided request draws what it draws alone
    solo = _engine(model, async_scheduling=async_sched)
    alone = solo.generate([[7, 9, 33, 7]], SamplingParams(max_tokens=16, temperature=1.0, seed=7,
                                                          ignore_eos=True))[0]
    assert alone.output_ids == seqs[2].output_ids


def test_cpu_engine_guided_preemption_resumes_the_state(model):
    eng = _engine(model, async_scheduling=True, num_blocks=24, max_num_seqs=4)
    eng.blocks.watermark_blocks = 0
    pat = r"[ab]{12}(cd|ef){4}"
    seqs = [eng.add_request([5 + i] * 12, SamplingParams(max_tokens=30, temperature=1.0, seed=i,
                                                         guided={"regex": pat}))
            for i in range(4)]
    while eng.has_work:
        eng.step()
    assert eng.scheduler.num_preemptions > 0
    g = G.compile_guided("regex", pat)
    for s in seqs:
        assert s.output_ids[-1] == eng.eos_id and len(s.output_ids) == 21
        assert g.matches(eng.tokenizer.decode(s.output_ids[:-1]).encode())
    assert eng.guided_state.num_free == 4 and eng.blocks.num_free == eng.blocks.num_blocks


def test_guided_cache_lru_keeps_tables_in_use():
    def table(n):
        return G.TokenTable(None, torch.zeros(n, 512, dtype=torch.int16), np.ones(n, bool))
    c = G.GuidedCache(3 * 1024)
    a = c.get("a", lambda: table(1))
    a.refs = 1
    c.get("b", lambda: table(1))
    c.get("c", lambda: table(1))
    assert list(c.tables) == ["a", "b", "c"] and c.hits == 0
    c.get("b", lambda: table(1))
    assert c.hits == 1
    c.get("d", lambda: table(1))          # over the bound: 'c' goes (least recent, unused)
    assert list(c.tables) == ["a", "b", "d"]
    c.get("e", lambda: table(2))          # 'a' is in use: never evicted
    assert "a" in c.tables and "e" in c.tables and c.nbytes <= 3 * 1024 + 2048
