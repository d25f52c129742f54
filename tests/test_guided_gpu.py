"""Guided decoding on the device: the grammar mask and the automaton-state update of the per-row
sampler entry (kernels/sampling_rows.hip) against torch references, then the engine paths on the
tiny model (async scheduling, graphs, preemption, slot reuse)."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
BF16 = torch.bfloat16
NINF = -float("inf")


@pytest.fixture(autouse=True)
def _native():
    from lumen.ops._native import native, native_error

    assert native() is not None, f"native extension must load on the GPU box: {native_error()!r}"
    torch.manual_seed(0)


def _C():
    from lumen.ops._native import native

    return native()


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32, device=DEV)


def _i64(x):
    return torch.as_tensor(x, dtype=torch.int64, device=DEV)


def _call(logits, temp, top_p=None, top_k=None, seed=None, offset=None, rngrow=None, **kw):
    R = logits.shape[0]
    out = torch.empty(R, device=DEV, dtype=torch.int64)
    lp = torch.empty(R, device=DEV, dtype=F32)
    tau = torch.empty(R, device=DEV, dtype=F32)
    _C().sample_rows(logits, temp,
                     torch.ones(R, device=DEV) if top_p is None else top_p,
                     torch.zeros(R, device=DEV, dtype=torch.int32) if top_k is None else top_k,
                     _i64([1] * R) if seed is None else seed,
                     _i64([0] * R) if offset is None else offset,
                     torch.arange(R, device=DEV) if rngrow is None else rngrow,
                     out_tokens=out, out_logprob=lp, out_tau=tau, **kw)
    return out, lp, tau


def _tie_free(R, V, dtype, g):
    """[R, V] logits whose values within a row have pairwise distinct bit patterns AFTER the
    rounding to ``dtype`` (and no -0 / +0 pair): every arg-max is unique."""
    if dtype == BF16:
        # sign | exponent field 63..190 (2^-64 .. 2^64) | 7 mantissa bits: 32768 distinct values
        e = torch.arange(63, 191).repeat_interleave(128)
        m = torch.arange(128).repeat(128)
        mag = (e << 7) | m
        pool = torch.cat([mag, mag | 0x8000])
        pool = torch.where(pool >= 0x8000, pool - 0x10000, pool).to(torch.int16)
        assert pool.numel() >= V
        rows = [pool[torch.randperm(pool.numel(), generator=g)[:V]] for _ in range(R)]
        return torch.stack(rows).view(BF16)
    rows = []
    for _ in range(R):
        idx = torch.randperm(1 << 20, generator=g)[:V]
        sign = torch.randint(0, 2, (V,), generator=g)
        bits = (118 << 23) + idx * 64 + (sign << 31)          # |x| in [2^-9, 2^-1)
        bits = torch.where(bits >= (1 << 31), bits - (1 << 32), bits).to(torch.int32)
        rows.append(bits.view(F32))
    return torch.stack(rows)


# ---- 1. greedy exactness ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("V", [515, 32000, 32768])
def test_greedy_masked_argmax_and_state(V, dtype):
    """Six greedy rows over one 5-state table whose states allow 1 token, ~1 %, ~50 %, every
    token and another ~50 %; rows 2 and 4 are unguided.  The guided rows sit in states 0, 1, 2
    and 3; in each state that forbids anything (0, 1, 2) the row's unconstrained arg-max is
    forbidden (the state that allows every token cannot forbid it).  Token = arg-max over the
    allowed set, new state = next[s][token], and the unguided rows are bitwise what the call
    without the guided arguments returns.  V = 515 makes every second table row unaligned,
    V = 32768 is the LDS limit."""
    R, S, G = 6, 5, 8
    g = torch.Generator().manual_seed(V + (dtype == BF16))
    logits = _tie_free(R, V, dtype, g)
    x = logits.float()
    am = x.argmax(-1)
    frac = [None, 0.01, 0.5, 1.0, 0.5]
    allowed = torch.zeros(S, V, dtype=torch.bool)
    for s in range(1, S):
        allowed[s] = torch.rand(V, generator=g) < frac[s] if frac[s] < 1.0 else True
    rows_state = {0: 0, 1: 1, 3: 2, 5: 3}
    slot_of = {0: 3, 1: 0, 3: 5, 5: 1}
    for r, s in rows_state.items():
        if s == 0:
            allowed[0, (int(am[r]) + 7) % V] = True      # the one allowed token: not the arg-max
        elif s != 3:
            allowed[s, am[r]] = False
    assert [int(allowed[s].sum()) for s in (0, 3)] == [1, V]
    nxt = torch.where(allowed, torch.randint(0, S, (S, V), generator=g), torch.tensor(-1))
    nxt = nxt.to(torch.int16).to(DEV)
    g_table = _i64([nxt.data_ptr() if r in rows_state else 0 for r in range(R)])
    g_slot = _i32([slot_of.get(r, -1) for r in range(R)])
    state = torch.full((G,), 4, dtype=torch.int32)
    for r, s in rows_state.items():
        state[slot_of[r]] = s
    before = state.clone()
    state = state.to(DEV)
    lg = logits.to(DEV)
    zero = torch.zeros(R, device=DEV)
    plain = _call(lg, zero)
    out, lp, tau = _call(lg, zero, g_table=g_table, g_slot=g_slot, g_state=state)
    out_h, nx_h = out.cpu(), nxt.cpu()
    for r in range(R):
        if r in rows_state:
            s = rows_state[r]
            if s != 3:
                assert not allowed[s, am[r]]
            want = torch.where(allowed[s], x[r], torch.tensor(NINF)).argmax()
            assert int(out_h[r]) == int(want), (r, s)
            before[slot_of[r]] = int(nx_h[s, want])
            # the log-probability is that of the masked distribution
            ref_lp = torch.log_softmax(torch.where(allowed[s], x[r].double(),
                                                   torch.tensor(NINF, dtype=torch.float64)), -1)
            assert abs(float(lp[r]) - float(ref_lp[want])) <= 1e-3 * (1 + abs(float(ref_lp[want])))
        else:
            assert int(out_h[r]) == int(am[r])
            assert int(out[r]) == int(plain[0][r])
            for a, b in zip((lp, tau), plain[1:]):
                assert torch.equal(a[r:r + 1].view(torch.int32), b[r:r + 1].view(torch.int32))
    assert torch.equal(state.cpu(), before)


# ---- 2. a state that allows EOS only --------------------------------------------------------------
@pytest.mark.parametrize("V", [515, 32000])
def test_only_eos_state(V):
    """Greedy and sampled rows, under top-k / top-p / min_p of every kind, in a state whose one
    allowed token is EOS: the token is EOS and the state stays."""
    EOS = 2
    R = 8
    g = torch.Generator().manual_seed(V)
    logits = (torch.randn(R, V, generator=g) * 3).to(BF16).to(DEV)
    nxt = torch.full((2, V), -1, dtype=torch.int16)
    nxt[0, 5:50] = 1
    nxt[1, EOS] = 1
    nxt = nxt.to(DEV)
    state = _i32([1] * R)
    temp = torch.tensor([0.0, 1.0, 0.7, 1.0, 2.0, 1.0, 0.3, 1.0], device=DEV)
    top_p = torch.tensor([1.0, 1.0, 0.5, 0.01, 1.0, 0.9, 1.0, 1.0], device=DEV)
    top_k = _i32([0, 0, 0, 0, 1, 5, 0, 40])
    min_p = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 0.1, 1.0, 0.5], device=DEV)
    out, lp, _ = _call(logits, temp, top_p, top_k, seed=_i64(list(range(R))), min_p=min_p,
                       g_table=_i64([nxt.data_ptr()] * R), g_slot=_i32(list(range(R))),
                       g_state=state)
    assert out.tolist() == [EOS] * R
    assert state.tolist() == [1] * R
    assert torch.allclose(lp.cpu(), torch.zeros(R), atol=1e-6)   # the only token: probability 1


# ---- 3. distribution ------------------------------------------------------------------------------
def test_masked_distribution_chi2():
    """65,536 rows of one V = 200 distribution at T = 0.8, each with its own seed and its own
    state slot, 60 tokens allowed: no draw outside the allowed set, a chi-square test against
    the renormalised masked softmax (the bound of the min_p test), every state advanced."""
    from scipy.stats import chisquare

    R, V, T = 65536, 200, 0.8
    g = torch.Generator().manual_seed(5)
    row = torch.randn(V, generator=g) * 2.0
    allow = torch.zeros(V, dtype=torch.bool)
    allow[torch.randperm(V, generator=g)[:60]] = True
    nxt = torch.full((2, V), -1, dtype=torch.int16)
    nxt[0, allow] = 1
    nxt[1] = 1
    nxt = nxt.to(DEV)
    logits = row.expand(R, V).contiguous().to(DEV)
    state = torch.zeros(R, dtype=torch.int32, device=DEV)
    out, _, _ = _call(logits, torch.full((R,), T, device=DEV),
                      seed=torch.arange(R, device=DEV) + 1000, offset=_i64([9] * R),
                      rngrow=_i64([0] * R), g_table=_i64([nxt.data_ptr()] * R),
                      g_slot=torch.arange(R, device=DEV, dtype=torch.int32), g_state=state)
    cnt = torch.bincount(out.cpu(), minlength=V).double()
    assert cnt[~allow].sum() == 0
    zs = row.float() * (1.0 / torch.tensor(T, dtype=F32))
    pr = torch.softmax(zs.double(), -1)[allow]
    res = chisquare(cnt[allow].numpy(), (pr / pr.sum() * R).numpy())
    assert res.pvalue > 1e-4, res
    assert bool((state == 1).all())


# ---- 4. composition -------------------------------------------------------------------------------
def _ulp(m):
    e = torch.floor(torch.log2(m.clamp(min=2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 23)


@pytest.mark.parametrize("V", [515, 32000])
def test_mask_bias_penalties_compose(V):
    """The mask, then logit_bias, then the penalties through ``logits_process``: masked entries
    are exactly -inf whatever the bias and the penalties add; every other entry is within the
    bound of test_logits_process_vs_f64 (4 f32 ulp of the largest intermediate magnitude) of
    the f64 reference; the library's torch reference is the same function."""
    from lumen.serve.model_runner import process_logits_ref

    R, S = 5, 3
    g = torch.Generator().manual_seed(V)
    logits = (torch.randn(R, V, generator=g) * 3).clamp(-64, 64).to(BF16)
    kind = torch.randint(0, 6, (S, V), generator=g)
    n = torch.randint(1, 6, (S, V), generator=g)
    c64 = torch.where(kind == 0, torch.full_like(n, 1 << 31), torch.zeros_like(n))
    c64 = torch.where(kind == 1, n, c64)
    c64 = torch.where(kind == 2, n + (1 << 31), c64)
    counts = torch.where(c64 >= (1 << 31), c64 - (1 << 32), c64).to(torch.int32)
    slot = torch.tensor([2, 0, -1, 1, -1])
    rp = torch.tensor([1.3, 1.0, 1.3, 1.3, 1.0], dtype=F32)
    fp = torch.tensor([0.7, -0.5, 0.7, 0.0, 0.0], dtype=F32)
    pp = torch.tensor([0.0, 0.7, -0.5, -0.5, 0.0], dtype=F32)
    bias = [([1, 7, V - 1, 100], [5.0, NINF, -2.5, 100.0]), None, ([0, 3], [-100.0, 1.25]),
            ([2, 9, 11, 200], [NINF, 0.5, -0.75, 3.0]), None]
    ptr, idx, val = [0], [], []
    for e in bias:
        if e is not None:
            idx += e[0]
            val += e[1]
        ptr.append(len(idx))
    allowed = torch.rand(4, V, generator=g) < torch.tensor([0.5, 0.05, 1.0, 0.5])[:, None]
    allowed[0, [1, 100]] = False          # biased (+5, +100) and masked: stays -inf
    allowed[1, 9] = False
    nxt = torch.where(allowed, torch.tensor(0), torch.tensor(-1)).to(torch.int16).to(DEV)
    g_state_rows = [0, 3, None, 1, 2]     # row 2 unguided, row 4 in the all-allowed state
    gstate = _i32([0, 3, 1, 2])
    g_slot = _i32([0, 1, -1, 2, 3])
    g_table = _i64([0 if s is None else nxt.data_ptr() for s in g_state_rows])
    mask = [None if s is None else ~allowed[s] for s in g_state_rows]
    # f64 reference with the largest intermediate magnitude of every element
    x0 = logits.double()
    b = torch.zeros(R, V, dtype=torch.float64)
    for i, e in enumerate(bias):
        if e is not None:
            b[i, e[0]] = torch.tensor(e[1], dtype=F32).double()
    x1 = x0 + b
    c = torch.zeros(R, V, dtype=torch.int64)
    for i in range(R):
        if slot[i] >= 0:
            c[i] = c64[slot[i]]
    nn = (c & 0x7FFFFFFF).double()
    rpd, fpd, ppd = rp.double()[:, None], fp.double()[:, None], pp.double()[:, None]
    x2 = torch.where((c != 0) & (rpd != 1.0), torch.where(x1 > 0, x1 / rpd, x1 * rpd), x1)
    pen = fpd * nn + ppd * (nn > 0).double()
    x3 = torch.where(c != 0, x2 - pen, x2)
    masked = torch.zeros(R, V, dtype=torch.bool)
    for i, m in enumerate(mask):
        if m is not None:
            masked[i] = m
    ref = torch.where(masked, torch.tensor(NINF, dtype=torch.float64), x3)
    fin = torch.isfinite(ref)
    mag = torch.stack([t.abs() for t in (x0, torch.where(fin, x1, x0), torch.where(fin, x2, x0),
                                         (fpd * nn).abs(), pen, torch.where(fin, x3, x0))]).amax(0)
    tol = 4 * _ulp(mag)
    out = torch.empty(R, V, device=DEV, dtype=F32)
    _C().logits_process(logits.to(DEV), _i32(ptr), _i32(idx), torch.tensor(val, device=DEV),
                        _i32(slot), rp.to(DEV), fp.to(DEV), pp.to(DEV), counts.to(DEV), out,
                        g_table=g_table, g_slot=g_slot, g_state=gstate)
    got = out.cpu()
    assert bool((got[masked] == NINF).all()) and int(masked.sum()) > V
    assert torch.equal(got[~fin].double(), ref[~fin])
    err = (got.double() - ref).abs()[fin]
    worst = (err / tol[fin]).max().item()
    print(f"mask + bias + penalties V={V}: worst error {worst:.3f} of the 4-ulp bound")
    assert bool((err <= tol[fin]).all()), worst
    assert gstate.tolist() == [0, 3, 1, 2]            # logits_process never advances a state
    counts_rows = torch.zeros(R, V, dtype=torch.int64)
    counts_rows[:] = c
    lib = process_logits_ref(logits.double(), counts_rows, rp, fp, pp,
                             bias=[None if e is None else (e[0], torch.tensor(e[1], dtype=F32))
                                   for e in bias], mask=mask)
    assert torch.equal(torch.nan_to_num(lib, neginf=-1e300), torch.nan_to_num(ref, neginf=-1e300))


# ---- 5. a chain of launches with no host read ---------------------------------------------------
def test_on_device_chain():
    """24 launches back to back over pre-generated logits, the automaton states advanced by the
    kernel alone, with the compiled table of (ab|cd)e{2} over ByteTokenizer(512): each row's
    tokens spell a full match, then EOS only; the final states are the host walk's."""
    from lumen.data.tokenizer import ByteTokenizer
    from lumen.serve.guided import build_token_index, compile_guided, token_bytes

    tok = ByteTokenizer(512)
    gr = compile_guided("regex", r"(ab|cd)e{2}")
    nxt, live = build_token_index(gr.trans, gr.accept, token_bytes(tok), 512, tok.eos_token_id,
                                  DEV)
    assert live.all() and nxt.dtype == torch.int16 and nxt.is_cuda
    steps, R, V = 24, 6, 512
    g = torch.Generator().manual_seed(11)
    logits = (torch.randn(steps, R, V, generator=g) * 3).to(BF16).to(DEV)
    temp = torch.tensor([0.0, 1.0, 0.0, 0.8, 1.5, 1.0], device=DEV)
    state = torch.zeros(R, dtype=torch.int32, device=DEV)
    g_table = _i64([nxt.data_ptr()] * R)
    slots = [4, 2, 0, 5, 1, 3]
    g_slot = _i32(slots)
    outs = []
    for i in range(steps):
        out, _, _ = _call(logits[i], temp, seed=_i64(list(range(7, 7 + R))), offset=_i64([i] * R),
                          rngrow=_i64([0] * R), g_table=g_table, g_slot=g_slot, g_state=state)
        outs.append(out)
    toks = torch.stack(outs).cpu().T.tolist()            # the first host read
    final = state.cpu().tolist()
    seen = set()
    for r, ids in enumerate(toks):
        k = ids.index(tok.eos_token_id)
        text = bytes(t - tok.offset for t in ids[:k])
        assert gr.matches(text), (r, text)
        assert set(ids[k:]) == {tok.eos_token_id}
        assert final[slots[r]] == gr.walk(text)
        seen.add(text)
    assert seen <= {b"abee", b"cdee"}
    # the greedy rows take the arg-max over the allowed set at every step of the host walk
    nx_h, x = nxt.cpu(), logits.float().cpu()
    for r in (0, 2):
        st = 0
        for i in range(steps):
            t = int(torch.where(nx_h[st] >= 0, x[i, r], torch.tensor(NINF)).argmax())
            assert toks[r][i] == t, (r, i)
            st = int(nx_h[st, t])


# ---- 6. V > 32768 -----------------------------------------------------------------------------------
def test_large_vocab_route():
    """V = 32832: ``logits_process`` materialises the masked rows and ``sample_rows(pre=True)``
    (the no-LDS form) draws from them and still advances the states; the fused call takes the
    same route by itself."""
    R, V, S = 3, 32832, 3
    g = torch.Generator().manual_seed(7)
    logits = _tie_free(R, V, F32, g)
    x = logits.float()
    allowed = torch.rand(S, V, generator=g) < 0.3
    st_rows = [2, None, 0]
    for r, s in enumerate(st_rows):
        if s is not None:
            allowed[s, x[r].argmax()] = False
    nxt = torch.where(allowed, torch.randint(0, S, (S, V), generator=g), torch.tensor(-1))
    nxt = nxt.to(torch.int16).to(DEV)
    g_table = _i64([0 if s is None else nxt.data_ptr() for s in st_rows])
    g_slot = _i32([1, -1, 0])
    want = [int(x[r].argmax()) if s is None else
            int(torch.where(allowed[s], x[r], torch.tensor(NINF)).argmax())
            for r, s in enumerate(st_rows)]
    want_state = [int(nxt[0, want[2]]), int(nxt[2, want[0]])]
    lg = logits.to(DEV)
    zero = torch.zeros(R, device=DEV)
    state = _i32([0, 2])
    proc = torch.empty(R, V, device=DEV, dtype=F32)
    _C().logits_process(lg, out=proc, g_table=g_table, g_slot=g_slot, g_state=state)
    assert state.tolist() == [0, 2]
    assert torch.equal(proc[1].cpu(), x[1])
    assert bool((proc[0].cpu() == NINF).eq(~allowed[2]).all())
    out, _, _ = _call(proc, zero, pre=True, g_table=g_table, g_slot=g_slot, g_state=state)
    assert out.tolist() == want and state.tolist() == want_state
    state2 = _i32([0, 2])
    out2, _, _ = _call(lg, zero, g_table=g_table, g_slot=g_slot, g_state=state2)
    assert out2.tolist() == want and state2.tolist() == want_state


# ---- 7. engine ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from lumen.models import build_model

    m = build_model("tiny-llama-gqa", dtype=torch.bfloat16, device="cuda", init="random", seed=1)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 2:
                p.mul_(5.0)
    return m.eval()


def _engine(model, **kw):
    from lumen.serve.engine import EngineConfig, LLMEngine

    kw.setdefault("num_blocks", 128)
    kw.setdefault("use_graphs", False)
    return LLMEngine(EngineConfig(model="tiny-llama-gqa", device="cuda", max_model_len=512,
                                  block_size=16, **kw), model=model)


SCHEMA = {"type": "object", "properties": {"ok": {"type": "boolean"}, "k": {"enum": ["a", "b"]}},
          "required": ["ok", "k"]}
MIX = [("regex", r"(ab|cd)e{2}", 0.0, None), ("choice", ["yes", "yeah", "no"], 1.0, 5),
       (None, None, 1.0, 7), ("json", SCHEMA, 1.0, 9), (None, None, 1.0, 21),
       ("choice", ["yes", "yeah", "no"], 0.0, None)]
PROMPTS = [[5, 5, 5, 5] * 3, [9, 8, 7] * 4, list(range(3, 20)), [42, 43] * 6, [17, 4, 99, 23, 8],
           [100] * 7]


def _text(eng, s):
    assert s.finish_reason == "stop" and s.output_ids[-1] == eng.eos_id, s.output_ids
    return bytes(t - 3 for t in s.output_ids[:-1])


def _run_mix(model, guided, graphs):
    from lumen.serve.sequence import SamplingParams

    eng = _engine(model, async_scheduling=True, use_graphs=graphs, max_num_seqs=8)
    seqs = []
    for (kind, val, T, seed), p in zip(MIX, PROMPTS):
        if kind is None:
            sp = SamplingParams(max_tokens=40, temperature=T, seed=seed, ignore_eos=True)
        elif guided:
            sp = SamplingParams(max_tokens=32, temperature=T, seed=seed, guided={kind: val})
        else:
            sp = SamplingParams(max_tokens=32, temperature=T, seed=seed, ignore_eos=True)
        seqs.append(eng.add_request(p, sp))
    while eng.has_work:
        eng.step()
    assert eng.blocks.num_free == eng.blocks.num_blocks
    assert eng.guided_state.num_free == 8 and all(s.guided_slot == -1 for s in seqs)
    assert all(t.refs == 0 for t in eng.guided_cache.tables.values())
    return eng, seqs


@pytest.mark.parametrize("graphs", [False, True])
def test_engine_guided_mix_keeps_async_overlap(model, graphs):
    from lumen.serve.guided import canonical, compile_guided

    eng, seqs = _run_mix(model, True, graphs)
    assert eng.async_sched and eng.guided_state.state is not None
    plain_eng, plain = _run_mix(model, False, graphs)
    assert plain_eng.guided_state.state is None            # nothing guided: nothing allocated
    for (kind, val, _, _), s in zip(MIX, seqs):
        if kind is None:
            continue
        text = _text(eng, s)
        assert compile_guided(kind, canonical(kind, val)).matches(text), (kind, text)
        if kind == "choice":
            assert text in (b"yes", b"yeah", b"no")
        if kind == "json":
            obj = json.loads(text)
            assert isinstance(obj["ok"], bool) and obj["k"] in ("a", "b") and len(obj) == 2
    # the seeded unguided requests draw what they draw without guided neighbours
    for i in (2, 4):
        assert len(seqs[i].output_ids) == 40 and seqs[i].output_ids == plain[i].output_ids
    assert eng.guided_stats()["guided_requests"] == 4
    assert eng.guided_stats()["guided_cache_hits"] == 1    # the choice grammar, asked twice
    ov, ov_plain = eng.stats["overlapped_steps"], plain_eng.stats["overlapped_steps"]
    print(f"overlapped steps: guided {ov}, unguided {ov_plain} (graphs {graphs})")
    assert abs(ov - ov_plain) <= 2


def test_engine_guided_preemption(model):
    """A cache too small for four sequences that each grow by 31 tokens: the run preempts, a
    re-admitted sequence resumes from the state its host tokens walk to, every output is a full
    match, every slot and block comes back."""
    from lumen.serve.guided import compile_guided
    from lumen.serve.sequence import SamplingParams

    eng = _engine(model, async_scheduling=True, num_blocks=12, max_num_seqs=8)
    eng.blocks.watermark_blocks = 0
    prompts = [[5, 5, 5, 5] * 6, [9, 8, 7] * 9, list(range(3, 40)), [42, 43] * 12]
    pat = r"[ab]{20}(cd|ef){5}"
    seqs = [eng.add_request(p, SamplingParams(max_tokens=40, temperature=1.0, seed=i,
                                              guided={"regex": pat}))
            for i, p in enumerate(prompts)]
    while eng.has_work:
        eng.step()
    assert eng.scheduler.num_preemptions > 0
    gr = compile_guided("regex", pat)
    for s in seqs:
        assert gr.matches(_text(eng, s)) and len(s.output_ids) == 31
    assert eng.blocks.num_free == eng.blocks.num_blocks
    assert eng.guided_state.num_free == 8 and all(s.guided_slot == -1 for s in seqs)
    assert all(s.n_pending == 0 for s in seqs)


def test_engine_guided_slot_reuse(model):
    """More guided requests than max_num_seqs = 2, through the same two slots: each output is
    a full match of its own grammar."""
    from lumen.serve.guided import compile_guided
    from lumen.serve.sequence import SamplingParams

    pats = [r"(ab|cd)e{2}", r"[0-9]{3}-[a-c]{2}", r"(yes|yeah|no)", r"x{7}", r"[ab]{4}c"]
    eng = _engine(model, async_scheduling=True, max_num_seqs=2)
    seqs = [eng.add_request(p, SamplingParams(max_tokens=16, temperature=1.0, seed=i,
                                              guided={"regex": pat}))
            for i, (p, pat) in enumerate(zip(PROMPTS, pats))]
    while eng.has_work:
        eng.step()
    for s, pat in zip(seqs, pats):
        assert compile_guided("regex", pat).matches(_text(eng, s)), pat
    assert eng.guided_state.num_free == 2
    assert np.all([t.refs == 0 for t in eng.guided_cache.tables.values()])
