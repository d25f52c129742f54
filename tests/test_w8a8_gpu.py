"""fp8 activations x fp8 weights (--quantization ptpc_fp8) on the GPU: kernels/w8a8_gemm.hip's
activation quantizer bit for bit against ``quantize_fp8_tokens``, its three GEMM kernels on exact
integer data and on random bytes against the f32 definition, the ``linear_nt`` dispatch, and the
engine against the fake-quant oracle of tests/test_w8a8_cpu.py."""
import gc

import pytest
import torch

from tests.test_w8a8_cpu import PROMPTS, fake_quant_oracle, ptpc_model, rel, run_ptpc_engine

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FP8 = torch.float8_e4m3fn
GEMV_SHAPES = [(68, 688), (1032, 256), (260, 4112), (264, 4112)]   # test_w8_gemv's
TOL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}


# ---- act_quant_fp8 ------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("K", [16, 688, 4112])
@pytest.mark.parametrize("M", [1, 5, 67])
def test_act_quant_bit_identical(M, K, dt):
    """K = 16: one chunk; 688: fewer chunks than threads; 4112: two chunks for some threads.
    x is a view into a buffer 64 wider; one row is zero, one holds the dtype's maximum (M = 1:
    one call each)."""
    from lumen.ops._native import native
    from lumen.ops.quant import quantize_fp8_tokens

    g = torch.Generator().manual_seed(M * 131 + K)
    big = torch.finfo(dt).max
    for special in (("zero", "max") if M == 1 else ("both",)):
        xb = (torch.randn(M, K + 64, generator=g) * torch.logspace(-3, 2, M)[:, None]).to(dt)
        if special in ("zero", "both"):
            xb[1 % M, :K] = 0
        if special in ("max", "both"):
            xb[2 % M, (5 * K) // 7] = -big if K == 688 else big
        x = xb.to(DEV)[:, :K]
        xq = torch.full((M + 2, K), 0x55, dtype=torch.uint8, device=DEV)
        sx = torch.full((M + 2,), 777.0, device=DEV)
        native().act_quant_fp8(x, xq[:M].view(FP8), sx[:M])
        rq, rs = quantize_fp8_tokens(x.cpu())
        assert torch.equal(sx[:M].cpu(), rs), (special, (sx[:M].cpu() - rs).abs().max())
        assert torch.equal(xq[:M].cpu(), rq.view(torch.uint8)), special
        assert ((xq[:M] & 0x7F) != 0x7F).all()                       # no NaN encoding
        assert (xq[M:] == 0x55).all() and (sx[M:] == 777.0).all()    # nothing beyond the outputs
        if special in ("zero", "both"):
            assert ((xq[1 % M] & 0x7F) == 0).all() and torch.isfinite(sx[1 % M])
    # the torch definition on the GPU agrees with the CPU one
    gq, gs = quantize_fp8_tokens(x)
    assert torch.equal(gq.view(torch.uint8).cpu(), rq.view(torch.uint8)) and torch.equal(gs.cpu(), rs)
    out = torch.empty(M, K, dtype=FP8, device=DEV)
    with pytest.raises(Exception):       # misaligned base (8 bytes into a row)
        native().act_quant_fp8(xb.to(DEV)[:, 4:4 + K], out, sx[:M])
    if K > 16:
        with pytest.raises(Exception):   # ragged K
            native().act_quant_fp8(x[:, :K - 8], out[:, :K - 8].contiguous(), sx[:M])


# ---- operands -----------------------------------------------------------------------------------

_ints = {}


def int_case(M, N, K, dt):
    """Small integers in [-8, 8] by different, asymmetric formulas of (m, k) and (n, k), scales
    that are powers of two (2^-1 .. 2^-4 per row of x, 2^-3 .. 2^-8 per row of W): every sum is an
    integer below 2^24, so the f32 reference is exact and the kernel's result must EQUAL it
    rounded once.  Computed once per shape on the CPU in f64."""
    key = (M, N, K)
    if key not in _ints:
        m, n, k = torch.arange(M)[:, None], torch.arange(N)[:, None], torch.arange(K)[None, :]
        xi = (3 * m + 5 * k + m * k) % 17 - 8
        wi = (7 * n + 2 * k + (n * k) // 3 + 4) % 17 - 8
        sx = torch.pow(2.0, -(1.0 + torch.arange(M) % 4)).float()
        sw = torch.pow(2.0, -(3.0 + torch.arange(N) % 6)).float()
        acc = xi.double() @ wi.double().t()
        assert acc.abs().max() < 2 ** 24
        ref = (acc * sx.double()[:, None] * sw.double()[None, :]).float()
        _ints[key] = (xi.float().to(FP8).to(DEV), sx.to(DEV), wi.float().to(FP8).to(DEV),
                      sw.to(DEV), ref.to(DEV))
    xq, sx, wq, sw, ref = _ints[key]
    from lumen.ops.quant import QuantWeight

    return xq, sx, QuantWeight(wq, sw, dt, act="fp8"), ref.to(dt)


def rand_case(M, N, K, dt, g):
    """Random e4m3fn bytes on both sides (test_w8_gpu.rand_qw; NaN encodings excluded) with
    distinct scales: the x scales log-uniform over 2^-10 .. 2^-2, in the fp16 case over four
    binades placed so that max |y| = 3e4 (and the smallest rows and columns stay far above
    fp16's subnormals)."""
    from tests.test_w8_gpu import rand_qw

    w = rand_qw(N, K, dt, g)
    w.act = "fp8"
    b = torch.randint(0, 256, (M, K), generator=g, dtype=torch.int32)
    b = torch.where((b & 0x7F) == 0x7F, b - 1, b).to(torch.uint8)
    lo, hi = (-10.0, -2.0) if dt == torch.bfloat16 else (-6.0, -2.0)
    e = torch.linspace(lo, hi, M)[torch.randperm(M, generator=g)]
    sx = torch.pow(torch.tensor(2.0), e + 1e-3 * torch.rand(M, generator=g)).float().to(DEV)
    xq = b.to(DEV).view(FP8)
    if dt == torch.float16:
        top = ((xq.double() @ w.q.double().t()) * sx.double()[:, None]
               * w.scale.double()[None, :]).abs().max()
        sx = (sx.double() * (3e4 / top)).float()
    return xq, sx, w


def check(y, xq, sx, w, what):
    """The issue's bound on the product against the f32 definition (formed in f64), and the same
    bound with every row and column divided by its scale."""
    acc = xq.double() @ w.q.double().t()
    ref = acc * sx.double()[:, None] * w.scale.double()[None, :]
    assert y.shape == ref.shape and y.dtype == w.dtype, what
    assert w.dtype != torch.float16 or ref.abs().max() < 6e4, what
    r = rel(y.double(), ref)
    rn = rel(y.double() / sx.double()[:, None] / w.scale.double()[None, :], acc)
    print(what, "rel", r, "scale-normalised rel", rn)
    assert r < TOL[w.dtype], (what, r)
    assert rn < TOL[w.dtype], (what, rn)
    return r


def strided(t, pad):
    """``t`` as a view into a buffer ``pad`` columns wider."""
    b = torch.zeros(t.shape[0], t.shape[1] + pad, dtype=torch.uint8, device=t.device).view(t.dtype) \
        if t.dtype == FP8 else torch.zeros(t.shape[0], t.shape[1] + pad, dtype=t.dtype,
                                           device=t.device)
    b[:, :t.shape[1]].copy_(t)
    return b[:, :t.shape[1]]


# ---- the GEMV -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,K", GEMV_SHAPES)
def test_w8a8_gemv(N, K, dt):
    from lumen.ops._native import native
    from lumen.ops.gemm import w8a8_gemv

    g = torch.Generator().manual_seed(N * 7 + K)
    for M in (1, 2, 3, 4):
        xq, sx, w, ref = int_case(M, N, K, dt)
        yb = torch.full((6, N), 777.0, device=DEV, dtype=dt)
        w8a8_gemv(strided(xq, 48), sx, w, out=yb[:M])
        assert torch.equal(yb[:M], ref), ("gemv exact", N, K, M, dt)
        assert (yb[M:] == 777.0).all(), M              # rows beyond M untouched
        xq, sx, w = rand_case(M, N, K, dt, g)
        check(w8a8_gemv(xq, sx, w), xq, sx, w, ("gemv", N, K, M, dt))
    xq, sx, w = rand_case(5, N, K, dt, g)
    with pytest.raises(Exception):                     # M above the kernel's range
        native().w8a8_gemv(xq, sx, w.q, w.scale, torch.empty(5, N, device=DEV, dtype=dt))
    with pytest.raises(Exception):                     # xq rows at a stride that is not % 16
        native().w8a8_gemv(strided(xq[:2], 8), sx[:2], w.q, w.scale,
                           torch.empty(2, N, device=DEV, dtype=dt))


# ---- the decode kernel --------------------------------------------------------------------------

@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("bm", [64, 128, 256])
def test_w8a8_decode_gemm_variants(bm, form):
    """Every compiled (BM, BN) variant with both MFMA forms: M below / at the block height, a
    ragged last column tile and whole tiles, K with whole k128 steps (640) and a 48-byte tail
    (688), split-K 1 / 2 / 3 with the tile counters zero after each launch; exact integers, then
    random bytes."""
    from lumen.ops._native import native
    from lumen.ops.gemm import W8A8_BNS, dg_workspace, w8a8_decode_gemm

    g = torch.Generator().manual_seed(bm + form)
    dt = torch.bfloat16
    for bn in W8A8_BNS[bm]:
        for N in (3 * bn + 12, 2 * bn):
            for K in (640, 688):
                for M in (5, bm - 11, bm):
                    xq, sx, w, ref = int_case(M, N, K, dt)
                    rq, rs, rw = rand_case(M, N, K, dt, g)
                    for s in (1, 2, 3):
                        y = w8a8_decode_gemm(xq, sx, w, bm, bn, s, form)
                        assert torch.equal(y, ref), ("dgemm exact", bm, bn, N, K, M, s, form)
                        y = w8a8_decode_gemm(rq, rs, rw, bm, bn, s, form)
                        check(y, rq, rs, rw, ("dgemm", bm, bn, N, K, M, s, form))
                        if s > 1:
                            assert int(dg_workspace(DEV)[1].abs().sum()) == 0
    bn = W8A8_BNS[bm][0]
    # fp16 outputs, strided xq and y
    M, N, K = bm - 3, 3 * bn + 12, 688
    xq, sx, w, ref = int_case(M, N, K, torch.float16)
    yb = torch.full((M, N + 4), 777.0, device=DEV, dtype=torch.float16)
    w8a8_decode_gemm(strided(xq, 16), sx, w, bm, bn, 2, form, out=yb[:, :N])
    assert torch.equal(yb[:, :N], ref) and (yb[:, N:] == 777.0).all()
    rq, rs, rw = rand_case(M, N, K, torch.float16, g)
    check(w8a8_decode_gemm(rq, rs, rw, bm, bn, 2, form), rq, rs, rw, ("dgemm fp16", bm, bn, form))
    # refusals: M above the block height, S above K / 64, a ragged K
    y1 = torch.empty(bm + 1, N, device=DEV, dtype=torch.float16)
    xq1, sx1, _ = rand_case(bm + 1, N, K, torch.float16, g)
    with pytest.raises(Exception):
        native().w8a8_decode_gemm(xq1, sx1, rw.q, rw.scale, y1, None, None, bm, bn, 1, form)
    ws, cnt = dg_workspace(DEV)
    with pytest.raises(Exception):
        native().w8a8_decode_gemm(rq, rs, rw.q, rw.scale, torch.empty_like(ref), ws, cnt, bm, bn,
                                  K // 64 + 1, form)
    assert int(cnt.abs().sum()) == 0
    # (64, 256) is not a compiled variant: refused by name before any launch
    with pytest.raises(ValueError, match=r"\(bm, bn\) must be one of \(64, 64\)"):
        native().w8a8_decode_gemm(rq[:5], rs[:5], rw.q, rw.scale, torch.empty_like(ref[:5]), None,
                                  None, 64, 256, 1, form)


# ---- the large-M kernel -------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_w8a8_gemm_large_m(dt):
    """M just above the decode range and 2 BM + 37 (a ragged last row tile), N = 2 BN + 12 (a
    ragged last column tile), K = 256 (two whole k128 steps) and 688 (a 48-byte tail), strided xq
    and y."""
    from lumen.ops._native import native
    from lumen.ops.gemm import W8A8_GEMM_TILES, w8a8_gemm

    g = torch.Generator().manual_seed(17)
    for tm, tn in W8A8_GEMM_TILES:
        N = 2 * tn + 12
        for M in (257, 2 * tm + 37):
            for K in (256, 688):
                xq, sx, w, ref = int_case(M, N, K, dt)
                yb = torch.full((M + 1, N + 4), 777.0, device=DEV, dtype=dt)
                w8a8_gemm(strided(xq, 32), sx, w, out=yb[:M, :N])
                assert torch.equal(yb[:M, :N], ref), ("gemm exact", M, N, K, dt)
                assert (yb[:, N:] == 777.0).all() and (yb[M:] == 777.0).all()
                rq, rs, rw = rand_case(M, N, K, dt, g)
                check(w8a8_gemm(rq, rs, rw), rq, rs, rw, ("gemm", M, N, K, dt))
    with pytest.raises(Exception):                     # the decode range is not this kernel's
        native().w8a8_gemm(rq[:256], rs[:256], rw.q, rw.scale,
                           torch.empty(256, N, device=DEV, dtype=dt))


# ---- dispatch -----------------------------------------------------------------------------------

def test_linear_nt_dispatch(monkeypatch):
    """GEMV, decode kernel, large-M kernel and fallback through ``linear_nt`` with injected
    plans; every route within the kernels' bound of the definition (the fallback: twice, for its
    extra rounding of W * sw); LUMEN_W8=0 takes the fallback; act=None keeps today's routes."""
    import lumen.ops.gemm as gm
    from lumen.ops.activation import swiglu
    from lumen.ops.quant import QuantWeight, quantize_fp8_tokens
    from tests.test_w8_gpu import check as check_w8, rand_qw

    g = torch.Generator().manual_seed(11)
    N, K, dt = 1024, 688, torch.bfloat16
    routes = []
    for name in ("w8a8_gemv", "w8a8_decode_gemm", "w8a8_gemm", "w8a8_fallback"):
        def wrap(*a, _f=getattr(gm, name), _n=name, **kw):
            routes.append(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(gm, name, wrap)
    plans = {(N, K, 64): (64, 2), (N, K, 256): (64, 1), (N, K, 512): (128, 1)}
    w = rand_qw(N, K, dt, g)
    wa = QuantWeight(w.q, w.scale, dt, act="fp8")

    def run(x, on=True, p=plans):
        monkeypatch.setattr(gm, "W8", on)
        monkeypatch.setattr(gm, "_w8a8_plans", p)
        routes.clear()
        y = gm.linear_nt(x, wa)
        xq, sx = quantize_fp8_tokens(x)
        acc = xq.double() @ w.q.double().t()
        ref = acc * sx.double()[:, None] * w.scale.double()[None, :]
        r = rel(y.double(), ref)
        rn = rel(y.double() / sx.double()[:, None] / w.scale.double()[None, :], acc)
        assert y.dtype == dt and y.shape == ref.shape
        return list(routes), max(r, rn)

    want = {1: "w8a8_gemv", 4: "w8a8_gemv", 7: "w8a8_decode_gemm", 64: "w8a8_decode_gemm",
            100: "w8a8_fallback",          # the 128 bucket is not listed
            200: "w8a8_decode_gemm", 300: "w8a8_gemm", 700: "w8a8_fallback"}
    for M, route in want.items():
        x = torch.randn(M, K, generator=g).to(DEV, dt)
        got, err = run(x)
        print("linear_nt", M, got, err)
        assert got == [route], (M, got)
        assert err < (2 if route == "w8a8_fallback" else 1) * TOL[dt], (M, route, err)
        got, err = run(x, on=False)                     # LUMEN_W8=0
        assert got == ["w8a8_fallback"] and err < 2 * TOL[dt], (M, got, err)
        got, err = run(x, p={})                         # an empty table: GEMV or fallback
        assert got == ["w8a8_gemv" if M <= 4 else "w8a8_fallback"] and err < 2 * TOL[dt]
    # a view with a row stride the quant kernel refuses is copied, not refused
    xv = torch.randn(3, K + 4, generator=g).to(DEV, dt)[:, :K]
    got, err = run(xv)
    assert got == ["w8a8_gemv"] and err < TOL[dt]
    gu = torch.randn(3, 2 * K, generator=g).to(DEV, dt)
    monkeypatch.setattr(gm, "W8", True)
    assert torch.equal(gm.swiglu_linear_nt(gu, wa), gm.linear_nt(swiglu(gu), wa))
    # act=None: today's weight-only routes, none of the W8A8 ones and no activation quantizer
    quant_calls = []
    monkeypatch.setattr(gm, "act_quant_fp8", lambda x: quant_calls.append(1))
    routes.clear()
    for M in (1, 7, 300):
        x = torch.randn(M, K, generator=g).to(DEV, dt)
        check_w8(gm.linear_nt(x, w), x, w, ("act=None", M))
    assert routes == [] and quant_calls == []


# ---- engine -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def served():
    m = ptpc_model(torch.bfloat16, DEV)
    return m, fake_quant_oracle(m), fake_quant_oracle(m, f32=True)


def engine_checks(r, what):
    print(what, "d", r["d"], "bound", r["bound"], "max logits rel", max(r["rels"]), "rows",
          len(r["rels"]), "agreement", r["agree"], "left out", r["left_out"])
    assert len(r["rels"]) >= 10
    assert max(r["rels"]) < r["bound"], (max(r["rels"]), r["bound"])
    assert all(r["own"])
    assert r["left_out"] <= 0.25, r["left_out"]
    assert r["agree"] >= 0.9, r["agree"]


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("nprompts", [1, 3, 7])
def test_engine_ptpc_fp8_matches_fake_quant_oracle(served, nprompts, graphs):
    """1 / 3 / 7 concurrent prompts (the GEMV, the GEMV at M = 3, the fallback), eager and
    graph-captured.  The function is discontinuous -- a 16-bit rounding difference ahead of a
    quantizer can flip an e4m3 rounding -- so the logits bound is measured from the oracle alone:
    d = the largest per-row relative difference between the oracle in bf16 and the oracle with
    f32 activations, bound = max(3e-2, 2 d) (run_ptpc_engine); measured values are in
    profiles/w8a8_serve/README.md."""
    m, oracle, oracle32 = served
    engine_checks(run_ptpc_engine(m, oracle, oracle32, "cuda", nprompts, graphs),
                  ("engine", nprompts, graphs))


def test_engine_ptpc_fp8_kernels_under_graph_capture(served, monkeypatch):
    """The shipped plan table lists no tiny-preset shape, so plans are injected for all four
    projections (the down projection's K = 688 has a k tail) and for the 300-token prefill: 7
    concurrent prompts run the split-K decode kernel and its shared workspace inside the captured
    decode graph, and the prefill runs the large-M kernel."""
    import lumen.ops.gemm as gm

    monkeypatch.setattr(gm, "_w8a8_plans", {
        (512, 256, 64): (64, 2), (256, 256, 64): (64, 2), (1376, 256, 64): (128, 1),
        (256, 688, 64): (64, 3),
        (512, 256, 512): (128, 1), (256, 256, 512): (128, 1), (1376, 256, 512): (128, 1),
        (256, 688, 512): (128, 1)})
    calls, big = [], []
    orig, orig_big = gm.w8a8_decode_gemm, gm.w8a8_gemm

    def spy(xq, sx, w, bm, bn, s, form=None, out=None):
        calls.append((tuple(w.shape), xq.shape[0], bm, bn, s))
        return orig(xq, sx, w, bm, bn, s, form, out=out)

    def spy_big(xq, sx, w, out=None):
        big.append((tuple(w.shape), xq.shape[0]))
        return orig_big(xq, sx, w, out=out)
    monkeypatch.setattr(gm, "w8a8_decode_gemm", spy)
    monkeypatch.setattr(gm, "w8a8_gemm", spy_big)
    m, oracle, oracle32 = served
    r = run_ptpc_engine(m, oracle, oracle32, "cuda", 7, True)
    shapes = {(512, 256), (256, 256), (1376, 256), (256, 688)}
    assert {c[0] for c in calls} == shapes and {c[0] for c in big} == shapes
    assert any(c[4] > 1 for c in calls) and gm._dg_ws
    for _, cnt in gm._dg_ws.values():            # every stream's tile counters are zero again
        assert int(cnt.abs().sum()) == 0
    engine_checks(r, ("engine, injected plans", len(calls), len(big)))


def test_multi_lora_on_ptpc_fp8_base(tmp_path):
    """One un-merged adapter over a ptpc_fp8 base (graph-captured decode) vs merged-then-quantized
    weights; shape and threshold of test_multi_lora_on_quantized_base.  The reference is that
    test's: the dequantised base with the adapter merged, its merged weight split again into the
    fp8 base part, which sees the fake-quantized x, and the adapter's delta, which reads the
    un-quantized x as the serving path's adapter products do (with this adapter the delta is
    ten times the base weight: fake-quantizing its input too measured an agreement of 0.56)."""
    from lumen.lora import LoraConfig, apply_lora, load_adapter, merge_lora, save_adapter
    from lumen.models import build_model
    from lumen.serve.engine import EngineConfig, LLMEngine
    from lumen.serve.sequence import SamplingParams
    from lumen.ops.quant import quantize_fp8_tokens
    from tests.test_w8_gpu import PROJ, dequantized_copy
    from tests.test_w8a8_cpu import add_fake_quant_hooks

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
                                   quantization="ptpc_fp8",
                                   lora_modules={"ad": str(tmp_path / "ad")}), model=base())
    seqs = [multi.add_request(p, SamplingParams(**vars(sp)), lora="ad" if i != 1 else None)
            for i, p in enumerate(prompts)]
    while multi.has_work:
        multi.step()
    torch.cuda.synchronize()
    del multi                       # its captured graphs go now, not inside a later capture
    gc.collect()
    plain = dequantized_copy(base())
    merged_m = dequantized_copy(base())
    load_adapter(merged_m, str(tmp_path / "ad"))
    merge_lora(merged_m)

    def split(lin, wq):
        delta = (lin.weight.float() - wq.float()).to(wq.dtype)

        def forward(x):
            xq, sx = quantize_fp8_tokens(x.reshape(-1, x.shape[-1]))
            fq = (xq.float() * sx[:, None]).to(x.dtype).view(x.shape)
            return torch.nn.functional.linear(fq, wq) + torch.nn.functional.linear(x, delta)
        lin.forward = forward

    for Lp, Lm in zip(plain.layers, merged_m.layers):
        for name in PROJ:
            split(Lm.get_submodule(name), Lp.get_submodule(name).weight)
    add_fake_quant_hooks(plain)
    for i, (p, s) in enumerate(zip(prompts, seqs)):
        ref_m = plain if i == 1 else merged_m
        ids = torch.tensor([p + s.output_ids[:-1]], device=DEV)
        with torch.no_grad():
            full = ref_m(ids).float().view(ids.shape[1], -1)
        ref = full[len(p) - 1:].argmax(-1).tolist()
        agree = sum(int(a == b) for a, b in zip(ref, s.output_ids)) / len(ref)
        print("multi-lora", i, agree)
        assert agree >= 0.85, (i, agree)
