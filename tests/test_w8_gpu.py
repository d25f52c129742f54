"""fp8 weight-only serving on the GPU: the three kernels of kernels/w8_gemm.hip against an f32
reference, the ``linear_nt`` dispatch, and the engine with ``quantization="fp8"`` against the full
forward of the model carrying the same (dequantised) weights."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
PROJ = ("self_attn.qkv_proj", "self_attn.o_proj", "mlp.gate_up_proj", "mlp.down_proj")


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def rand_qw(N, K, dt, g):
    """Random e4m3fn bytes (the two NaN encodings excluded) and per-row scales log-uniform over
    2^-12 .. 2^-2, all distinct: a missing, transposed or mis-indexed scale fails loudly."""
    from lumen.ops.quant import QuantWeight

    b = torch.randint(0, 256, (N, K), generator=g, dtype=torch.int32)
    b = torch.where((b & 0x7F) == 0x7F, b - 1, b).to(torch.uint8)
    e = torch.linspace(-12.0, -2.0, N)[torch.randperm(N, generator=g)]
    s = torch.pow(torch.tensor(2.0), e + 1e-3 * torch.rand(N, generator=g)).float()
    assert s.unique().numel() == N
    return QuantWeight(b.to(DEV).view(torch.float8_e4m3fn), s.to(DEV), dt)


def check(y, x, qw, what):
    """The issue's bound on the whole product, and the same bound with every column divided by
    its scale (so the small-scale rows count as much as the large ones)."""
    ref = x.float() @ (qw.q.float() * qw.scale[:, None]).t()
    assert y.shape == ref.shape and y.dtype == x.dtype, what
    r = rel(y, ref)
    rn = rel(y.float() / qw.scale[None, :], ref / qw.scale[None, :])
    print(what, "rel", r, "scale-normalised rel", rn)
    assert r < 1e-2, (what, r)
    assert rn < 1e-2, (what, rn)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,K", [(68, 688), (1032, 256), (260, 4112), (264, 4112)])
def test_w8_gemv(N, K, dt):
    """(68, 688): fewer chunks than lanes, ragged K; (1032, 256): K below one wave step;
    (260, 4112): several steps plus a one-chunk tail, N % 16 != 0; (264, 4112): the same K on
    the 8-rows-per-workgroup form (N % 8 == 0; 68 and 260 take the 4-row form)."""
    from lumen.ops._native import native

    g = torch.Generator().manual_seed(N * 7 + K)
    qw = rand_qw(N, K, dt, g)
    for M in (1, 2, 3, 4):
        xb = torch.randn(M, K + 128, generator=g).to(DEV, dt)
        x = xb[:, :K]                                   # a view into a buffer 128 wider
        yb = torch.full((6, N), 777.0, device=DEV, dtype=dt)
        native().w8_gemv(x, qw.q, qw.scale, yb[:M])
        check(yb[:M], x, qw, ("gemv", N, K, M, dt))
        assert (yb[M:] == 777.0).all(), M              # rows beyond M untouched
    with pytest.raises(Exception):
        native().w8_gemv(torch.zeros(5, K, device=DEV, dtype=dt), qw.q, qw.scale,
                         torch.empty(5, N, device=DEV, dtype=dt))


@pytest.mark.parametrize("bm", [64, 128, 256])
def test_w8_decode_gemm_variants(bm):
    """Every compiled (BM, BN) variant: M below / at the block height, a ragged last column tile
    and whole tiles, split-K 1 / 2 / 3 with the tile counters zero after each launch, strided x."""
    from lumen.ops._native import native
    from lumen.ops.gemm import W8_BNS, dg_workspace, w8_decode_gemm

    g = torch.Generator().manual_seed(bm)
    K = 640
    for bn in W8_BNS[bm]:
        for N in (3 * bn + 12, 2 * bn):
            qw = rand_qw(N, K, torch.bfloat16, g)
            for M in (5, bm - 11, bm):
                xb = torch.randn(M, K + 64, generator=g).to(DEV, torch.bfloat16)
                x = xb[:, :K]                           # row stride K + 64
                for s in (1, 2, 3):
                    y = w8_decode_gemm(x, qw, bm, bn, s)
                    check(y, x, qw, ("dgemm", bm, bn, N, M, s))
                    if s > 1:
                        assert int(dg_workspace(DEV)[1].abs().sum()) == 0
    bn = W8_BNS[bm][0]
    # fp16 operands
    qw = rand_qw(3 * bn + 12, K, torch.float16, g)
    x = torch.randn(bm - 3, K, generator=g).to(DEV, torch.float16)
    y = w8_decode_gemm(x, qw, bm, bn, 2)
    check(y, x, qw, ("dgemm fp16", bm, bn))
    # a split-K launch on a side stream gets a workspace of its own and the same result
    main_ws = dg_workspace(DEV)[0].data_ptr()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y2 = w8_decode_gemm(x, qw, bm, bn, 2)
        assert dg_workspace(DEV)[0].data_ptr() != main_ws
        assert int(dg_workspace(DEV)[1].abs().sum()) == 0
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(y2, y)
    # M above the block height fails loudly
    with pytest.raises(Exception):
        native().w8_decode_gemm(torch.zeros(bm + 1, K, device=DEV, dtype=torch.float16), qw.q,
                                qw.scale, torch.empty(bm + 1, qw.shape[0], device=DEV,
                                                      dtype=torch.float16), None, None, bm, bn, 1)
    # (64, 256) is not a compiled variant: refused by name before any launch
    with pytest.raises(ValueError, match=r"\(bm, bn\) must be one of \(64, 64\)"):
        native().w8_decode_gemm(x[:5], qw.q, qw.scale, torch.empty_like(y[:5]), None, None, 64,
                                256, 1)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,K", [(68, 688), (4100, 272)])
def test_w8_dequant_bit_identical(N, K, dt):
    from lumen.ops.gemm import w8_dequant

    qw = rand_qw(N, K, dt, torch.Generator().manual_seed(N + K))
    out = torch.empty(N, K, device=DEV, dtype=dt)
    w8_dequant(qw, out)
    assert torch.equal(out, qw.dequant())
    assert torch.equal(w8_dequant(qw), qw.dequant())   # the persistent scratch


def test_linear_nt_dispatch(monkeypatch):
    """All three routes at (N, K) = (1024, 688) -- a K the MFMA kernel refuses -- and the MFMA
    route itself at K = 640 through an injected plan; LUMEN_W8=0 gives the same within the bound."""
    import lumen.ops.gemm as gm
    from lumen.ops.activation import swiglu

    g = torch.Generator().manual_seed(11)
    for K, plans in ((688, {}), (640, {(1024, 640, 64): (64, 2), (1024, 640, 128): (128, 1)})):
        qw = rand_qw(1024, K, torch.bfloat16, g)
        for M in (1, 4, 7, 64, 100, 300):
            x = torch.randn(M, K, generator=g).to(DEV, torch.bfloat16)
            for on in (True, False):
                monkeypatch.setattr(gm, "W8", on)
                monkeypatch.setattr(gm, "_w8_plans", plans)
                assert (gm.w8_plan(x, qw) is not None) == (4 < M <= 256 and bool(plans))
                check(gm.linear_nt(x, qw), x, qw, ("linear_nt", K, M, on))
        gu = torch.randn(3, 2 * K, generator=g).to(DEV, torch.bfloat16)
        check(gm.swiglu_linear_nt(gu, qw), swiglu(gu), qw, ("swiglu_linear_nt", K))
        # a one-row view whose row stride is below K: refused by the predicate, not the binding
        monkeypatch.setattr(gm, "W8", True)
        x1 = torch.as_strided(torch.randn(K, generator=g).to(DEV, torch.bfloat16), (1, K), (8, 1))
        assert not gm.w8_gemv_ok(x1, qw)
        check(gm.linear_nt(x1, qw), x1, qw, ("linear_nt one-row view", K))
    # the shipped table only lists compiled variants
    monkeypatch.setattr(gm, "_w8_plans", None)
    for (N, K, bm), (bn, s) in gm.w8_plans().items():
        assert bm in gm.W8_BNS and bn in gm.W8_BNS[bm] and 1 <= s <= K // 64 and K % 64 == 0


# ---- engine -------------------------------------------------------------------------------------

def dequantized_copy(m):
    """A copy of ``m`` whose projection weights are replaced by their fp8 round trip: the oracle
    carries the same rounded weights as the quantized engine."""
    from lumen.ops.quant import quantize_fp8_rows

    d = copy.deepcopy(m)
    with torch.no_grad():
        for L in d.layers:
            for name in PROJ:
                lin = L.get_submodule(name)
                lin.weight.copy_(quantize_fp8_rows(lin.weight).dequant())
    return d.eval()


@pytest.fixture(scope="module")
def gqa():
    from lumen.models import build_model

    m = build_model("tiny-llama-gqa", dtype=torch.bfloat16, device=DEV, init="random", seed=3)
    m.eval()
    return m, dequantized_copy(m)


PROMPTS = [[(11 * i + 5) % 500 + 3 for i in range(300)],   # a prefill step on the scratch path
           [5, 9, 33, 7] * 10, list(range(3, 60)), [42, 43], list(range(100, 131)),
           [7, 8, 9, 10, 11, 12], list(range(200, 245))]


def run_engine(m, oracle, nprompts, graphs, kv="auto", max_tokens=12, keep=False):
    """Greedy agreement with the oracle's teacher-forced argmax per sequence, and the decode
    logits' relative error per (step, row) against the oracle's full forward."""
    from lumen.ops.quant import QuantWeight
    from lumen.serve.engine import EngineConfig, LLMEngine
    from lumen.serve.sequence import SamplingParams

    eng = LLMEngine(EngineConfig(model="tiny-llama-gqa", device="cuda", max_model_len=512,
                                 block_size=16, num_blocks=128, use_graphs=graphs,
                                 quantization="fp8", kv_cache_dtype=kv), model=m)
    assert all(isinstance(w, QuantWeight) for L in eng.weights.layers
               for w in (L.qkv, L.o, L.gate_up, L.down))
    prompts = PROMPTS[:nprompts]
    seqs = [eng.add_request(p, SamplingParams(max_tokens=max_tokens, temperature=0.0,
                                              ignore_eos=True)) for p in prompts]
    got = []
    orig = eng.runner.decode

    def spy(inp):
        out = orig(inp)
        got.append((inp.tokens.clone(), inp.positions.clone(), out.float().clone()))
        return out
    eng.runner.decode = spy
    while eng.has_work:
        eng.step()
    torch.cuda.synchronize()
    agrees, fulls = [], []
    for p, s in zip(prompts, seqs):
        assert len(s.output_ids) == max_tokens
        ids = torch.tensor([p + s.output_ids[:-1]], device=DEV)
        with torch.no_grad():
            full = oracle(ids).float().view(ids.shape[1], -1)
        fulls.append((p + s.output_ids, full))
        ref = full[len(p) - 1:].argmax(-1).tolist()
        agrees.append(sum(int(a == b) for a, b in zip(ref, s.output_ids)) / len(ref))
    if keep:
        run_engine.last_outputs = [list(s.output_ids) for s in seqs]
    rels = []
    for toks, pos, lg in got:
        toks, pos = toks.tolist(), pos.tolist()
        for i in range(min(len(toks), lg.shape[0])):
            # the row's sequence: the one holding this token at this position
            owners = [full for ids, full in fulls
                      if pos[i] < full.shape[0] and ids[pos[i]] == toks[i]]
            if len(owners) == 1:
                rels.append(rel(lg[i], owners[0][pos[i]]))
    return agrees, rels


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("nprompts", [1, 3, 7])
def test_engine_fp8_matches_dequantized_forward(gqa, nprompts, graphs):
    """1 / 3 / 7 concurrent prompts: the GEMV, the GEMV at M = 3, and the MFMA-or-fallback
    route, eager and graph-captured; thresholds of test_engine_decode_matches_full_forward and
    test_decode_logits_close_to_full_forward."""
    m, oracle = gqa
    agrees, rels = run_engine(m, oracle, nprompts, graphs)
    print("agreement", agrees, "max logits rel", max(rels), "rows", len(rels))
    assert len(rels) >= 10
    assert min(agrees) >= 0.9, agrees
    assert max(rels) < 3e-2, max(rels)


def teacher_forced_choices(model, prompts, forced, kv):
    """An unquantized engine on ``model`` (synchronous scheduling) that is fed the tokens
    ``forced[i]`` of another engine instead of its own samples: returns, per prompt, the tokens
    it would have chosen itself at every position (teacher-forced greedy)."""
    from lumen.serve.engine import EngineConfig, LLMEngine
    from lumen.serve.sequence import SamplingParams

    eng = LLMEngine(EngineConfig(model="tiny-llama-gqa", device="cuda", max_model_len=512,
                                 block_size=16, num_blocks=128, use_graphs=True,
                                 async_scheduling=False, kv_cache_dtype=kv), model=model)
    n = len(forced[0])
    seqs = [eng.add_request(p, SamplingParams(max_tokens=n, temperature=0.0, ignore_eos=True))
            for p in prompts]
    index = {s.seq_id: i for i, s in enumerate(seqs)}
    chosen = [[] for _ in seqs]
    state = {}
    build, sample = eng._build_input, eng.runner.sample

    def spy_build(batch):
        state["rows"] = list(batch.sampled)
        return build(batch)

    def spy_sample(*a, **kw):
        t, lp = sample(*a, **kw)
        own = t.tolist()
        t = t.clone()
        for r, sq in enumerate(state["rows"]):
            i = index[sq.seq_id]
            chosen[i].append(own[r])
            t[r] = forced[i][len(sq.output_ids)]
        return t, lp
    eng._build_input, eng.runner.sample = spy_build, spy_sample
    while eng.has_work:
        eng.step()
    for s, f in zip(seqs, forced):
        assert s.output_ids == f       # the reference really followed the forced tokens
    return chosen


def test_engine_fp8_weights_and_fp8_kv(gqa):
    """Both fp8 features together.  Logits: against the full forward of the dequantised model,
    with test_fresh_prompt_prefill_matches_paged's bound for an fp8 cache (the decode rows read
    e4m3-rounded K/V, the oracle 16-bit).  Tokens: greedy agreement >= 0.9, teacher-forced,
    against an engine that shares the cache rounding -- the dequantised model served unquantized
    with the same fp8 cache -- so that only the weight path differs between the two sides.
    (Against the 16-bit-cache full forward the agreement measured 1.0 / 0.92 / 0.83 over 12
    tokens at a logits error of 0.036, 0.008 with a 16-bit cache: the cache rounding alone flips
    near-tie tokens of a random-init model.)"""
    m, oracle = gqa
    n = 20
    from lumen.serve.engine import EngineConfig, LLMEngine  # noqa: F401

    agrees, rels = run_engine(m, oracle, 3, True, kv="fp8", max_tokens=n, keep=True)
    outs = run_engine.last_outputs
    print("vs 16-bit-cache forward: agreement", agrees, "max logits rel", max(rels),
          "rows", len(rels))
    assert len(rels) >= 10
    assert max(rels) < 6e-2, max(rels)
    chosen = teacher_forced_choices(oracle, PROMPTS[:3], outs, "fp8")
    agree = [sum(int(a == b) for a, b in zip(c, o)) / len(o) for c, o in zip(chosen, outs)]
    print("vs fp8-cache engine on the dequantised model: agreement", agree)
    assert all(len(c) == n for c in chosen)
    assert min(agree) >= 0.9, agree


def test_engine_fp8_mfma_route_under_graph_capture(gqa, monkeypatch):
    """The shipped plan table lists no tiny-preset shape, so here a plan is injected for the
    q|k|v, o and gate|up projections (K = 256; the down projection's K = 688 stays on the
    fallback): 7 concurrent prompts run the split-K MFMA kernel and its shared workspace inside
    the captured decode graph."""
    import lumen.ops.gemm as gm

    monkeypatch.setattr(gm, "_w8_plans", {(512, 256, 64): (64, 2), (256, 256, 64): (64, 4),
                                          (1376, 256, 64): (128, 1)})
    calls = []
    orig = gm.w8_decode_gemm

    def spy(x, w, bm, bn, s, out=None):
        calls.append((tuple(w.shape), x.shape[0], bm, bn, s))
        return orig(x, w, bm, bn, s, out=out)
    monkeypatch.setattr(gm, "w8_decode_gemm", spy)
    m, oracle = gqa
    agrees, rels = run_engine(m, oracle, 7, True)
    print("agreement", agrees, "max logits rel", max(rels), "rows", len(rels), "mfma calls",
          len(calls))
    assert {c[0] for c in calls} == {(512, 256), (256, 256), (1376, 256)}
    assert any(c[4] > 1 for c in calls) and gm._dg_ws
    for _, cnt in gm._dg_ws.values():            # every stream's tile counters are zero again
        assert int(cnt.abs().sum()) == 0
    assert len(rels) >= 10
    assert min(agrees) >= 0.9, agrees
    assert max(rels) < 3e-2, max(rels)


def test_serve_weights_refuse_ragged_k_at_load():
    """K % 16 != 0 (here the down projection, K = 680) is refused when the weights are built,
    with a message that names the projection, not at the first step."""
    from lumen.models import build_model, get_config
    from lumen.serve.model_runner import ServeWeights

    cfg = get_config("tiny-llama-gqa")
    cfg.intermediate_size = 680
    m = build_model(cfg, dtype=torch.bfloat16, device=DEV, init="random", seed=1)
    ServeWeights(m, 0, 1)                                   # 16-bit weights: fine
    with pytest.raises(ValueError, match="K % 16"):
        ServeWeights(m, 0, 1, "fp8")


def test_multi_lora_on_quantized_base(tmp_path):
    """One un-merged adapter over an fp8 base (graph-captured decode) vs the dequantised model
    with that adapter merged; same shape and threshold as
    test_multi_lora_graph_decode_matches_merged."""
    from lumen.lora import LoraConfig, apply_lora, load_adapter, merge_lora, save_adapter
    from lumen.models import build_model
    from lumen.serve.engine import EngineConfig, LLMEngine
    from lumen.serve.sequence import SamplingParams

    def base():
        m = build_model("tiny-llama-gqa", dtype=torch.bfloat16, device=DEV, init="random", seed=3)
        with torch.no_grad():
            for p in m.parameters():
                if p.dim() == 2:
                    p.mul_(4.0)
        return m.eval()

    m = base()
    apply_lora(m, LoraConfig(r=16, lora_alpha=32))
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.requires_grad:
                p.copy_((torch.randn(p.shape, generator=g) * 0.2).to(DEV))
    save_adapter(m, str(tmp_path / "ad"), "tiny-llama-gqa")
    prompts = [[5, 9, 33, 7] * 10, list(range(3, 60)), [42, 43]]
    sp = SamplingParams(max_tokens=16, temperature=0.0, ignore_eos=True)
    multi = LLMEngine(EngineConfig(model="tiny-llama-gqa", device="cuda", max_model_len=512,
                                   block_size=16, num_blocks=128, use_graphs=True,
                                   quantization="fp8",
                                   lora_modules={"ad": str(tmp_path / "ad")}), model=base())
    seqs = [multi.add_request(p, SamplingParams(**vars(sp)), lora="ad" if i != 1 else None)
            for i, p in enumerate(prompts)]
    while multi.has_work:
        multi.step()
    plain = dequantized_copy(base())
    merged_m = dequantized_copy(base())
    load_adapter(merged_m, str(tmp_path / "ad"))
    merge_lora(merged_m)
    for i, (p, s) in enumerate(zip(prompts, seqs)):
        ref_m = plain if i == 1 else merged_m
        ids = torch.tensor([p + s.output_ids[:-1]], device=DEV)
        with torch.no_grad():
            full = ref_m(ids).float().view(ids.shape[1], -1)
        ref = full[len(p) - 1:].argmax(-1).tolist()
        agree = sum(int(a == b) for a, b in zip(ref, s.output_ids)) / len(ref)
        assert agree >= 0.85, (i, agree)
