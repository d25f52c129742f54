"""MXFP4 weights x fp8 activations (--quantization mxfp4) on the GPU: kernels/w4a8_gemm.hip's
dequantiser bit for bit against ``Mxfp4Weight.dequant``, its decode kernel on exact integer data
(which fixes the lane-to-k map of the mixed-format MFMA operands and the scale lane map) and on
random data against the f64 definition, the ``linear_nt`` dispatch, and the engine against the
fake-quant oracle of tests/test_mxfp4_cpu.py."""
import json

import pytest
import torch

from tests.test_mxfp4_cpu import engine_checks, mxfp4_oracle, run_mxfp4_engine
from tests.test_w8a8_cpu import ptpc_model, rel
from tests.test_w8a8_gpu import TOL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FP8 = torch.float8_e4m3fn
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def holder(codes, ebytes, K, dt):
    """Mxfp4Weight on the GPU from [N, Kp] codes (padding codes zeroed here) and [N, Kp / 32]
    scale bytes."""
    from lumen.ops.quant import Mxfp4Weight

    codes = codes.clone().to(torch.uint8)
    codes[:, K:] = 0
    q = (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()
    return Mxfp4Weight(q.to(DEV), ebytes.to(torch.uint8).contiguous().to(DEV), K, dt)


def wdq64(w):
    """The holder's weights in f64 on the CPU, formed here from the codes and the scale bytes."""
    q, s = w.q.cpu(), w.scale.cpu()
    codes = torch.stack((q & 0xF, q >> 4), dim=-1).view(q.shape[0], -1).long()
    lut = torch.tensor(GRID + tuple(-v for v in GRID), dtype=torch.float64)
    v = lut[codes].view(q.shape[0], -1, 32) * torch.pow(
        torch.tensor(2.0, dtype=torch.float64), (s.double() - 127))[:, :, None]
    return v.view(q.shape[0], -1)[:, :w.K]


# ---- w4_dequant ---------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,K", [(72, 400), (64, 4096)])
def test_w4_dequant_bit_identical(N, K, dt):
    """Random codes (negative zeros included), block exponents spread over -12 .. 2; a partial
    last block at K = 400; the scratch route and an explicit output; nothing past the output."""
    from lumen.ops.gemm import w4_dequant

    g = torch.Generator().manual_seed(N + K)
    Kp = -(-K // 32) * 32
    codes = torch.randint(0, 16, (N, Kp), generator=g)
    e = torch.randint(-12, 3, (N, Kp // 32), generator=g)
    e[0, :15] = torch.arange(-12, 3)[:min(15, Kp // 32)]
    w = holder(codes, e + 127, K, dt)
    want = w.dequant()
    assert want.dtype == dt and torch.equal(want.double().cpu(), wdq64(w))   # exact in 16 bits
    buf = torch.full((N * K + 64,), 777.0, device=DEV, dtype=dt)
    w4_dequant(w, out=buf[:N * K].view(N, K))
    assert torch.equal(buf[:N * K].view(N, K).view(torch.int16), want.view(torch.int16))
    assert (buf[N * K:] == 777.0).all()
    assert torch.equal(w4_dequant(w).view(torch.int16), want.view(torch.int16))


# ---- the decode kernel --------------------------------------------------------------------------

_ints = {}


def int_case(M, dt, N=72, K=400):
    """Codes and block exponents by asymmetric integer formulas of (n, k) and (n, block)
    (exponents in {-1, 0, 1, 2}), xq integers in [-8, 8] by a different formula of (m, k), sx
    powers of two: 4 * wdq is an integer of magnitude <= 96, so four times every sum is an integer
    below 2^24 (asserted), f32 accumulation is exact and y must EQUAL the f64 reference rounded
    once.  K = 400: the last block (16 k) and the last k128 step are both partial."""
    if M not in _ints:
        n, k = torch.arange(N)[:, None], torch.arange(-(-K // 32) * 32)[None, :]
        m, b = torch.arange(M)[:, None], torch.arange(-(-K // 32))[None, :]
        codes = (5 * n + 3 * k + (n * k) // 7 + 1) % 16
        e = (3 * n + 2 * b + (n * b) // 5) % 4 - 1
        xi = (3 * m + 5 * k[:, :K] + m * k[:, :K]) % 17 - 8
        sx = torch.pow(2.0, -(1.0 + torch.arange(M) % 4)).float()
        _ints[M] = (codes, e + 127, xi.float().to(FP8).to(DEV), sx.to(DEV))
    codes, eb, xq, sx = _ints[M]
    w = holder(codes, eb, K, dt)
    acc = xq.double().cpu() @ wdq64(w).t()
    assert (4 * acc == (4 * acc).round()).all() and 4 * acc.abs().max() < 2 ** 24
    return xq, sx, w, (acc * sx.double().cpu()[:, None]).to(dt).to(DEV)


@pytest.mark.parametrize("bm", [16, 64, 128, 256])
def test_w4a8_decode_gemm_exact_integers(bm):
    """Every compiled (BM, BN) at every M <= BM of the list, split-K 1 and 3, N = 72 (a partial
    16-row tile, not a multiple of any BN); the output buffer is wider than N and its sentinel
    survives; the tile counters are zero after every split-K launch."""
    from lumen.ops.gemm import W4A8_BNS, dg_workspace, w4a8_decode_gemm

    for dt in (torch.bfloat16, torch.float16):
        for M in (m for m in (1, 3, 16, 17, 64, 200) if m <= bm):
            xq, sx, w, ref = int_case(M, dt)
            for bn in W4A8_BNS[bm]:
                for s in (1, 3):
                    yb = torch.full((M + 1, 72 + 8), 777.0, device=DEV, dtype=dt)
                    w4a8_decode_gemm(xq, sx, w, bm, bn, s, out=yb[:M, :72])
                    assert torch.equal(yb[:M, :72], ref), ("exact", bm, bn, M, s, dt)
                    assert (yb[:, 72:] == 777.0).all() and (yb[M:] == 777.0).all()
                    if s > 1:
                        assert int(dg_workspace(DEV)[1].abs().sum()) == 0


def rand_case(M, N, K, dt, g):
    """Random codes and scale bytes 2^-10 .. 2^-4, random e4m3 bytes for xq (NaN encodings
    excluded), distinct sx (log-uniform over 2^-6 .. 2^-2: max |y| stays inside fp16)."""
    Kp = -(-K // 32) * 32
    w = holder(torch.randint(0, 16, (N, Kp), generator=g),
               torch.randint(117, 124, (N, Kp // 32), generator=g), K, dt)
    b = torch.randint(0, 256, (M, K), generator=g, dtype=torch.int32)
    b = torch.where((b & 0x7F) == 0x7F, b - 1, b).to(torch.uint8)
    e = torch.linspace(-6.0, -2.0, M)[torch.randperm(M, generator=g)]
    sx = torch.pow(torch.tensor(2.0), e + 1e-3 * torch.rand(M, generator=g)).float()
    if dt == torch.float16:
        top = ((b.view(FP8).double() @ wdq64(w).t()) * sx.double()[:, None]).abs().max()
        sx = (sx.double() * min(1.0, 3e4 / top)).float()
    return b.to(DEV).view(FP8), sx.to(DEV), w


def check(y, xq, sx, w, what, tol=1.0):
    """The product against the definition formed in f64: the same accumulation and the same
    single output rounding."""
    ref = (xq.double().cpu() @ wdq64(w).t()) * sx.double().cpu()[:, None]
    assert y.shape == ref.shape and y.dtype == w.dtype, what
    assert w.dtype != torch.float16 or ref.abs().max() < 6e4, what
    r = rel(y.double().cpu(), ref)
    print(what, "rel", r)
    assert r < tol * TOL[w.dtype], (what, r)
    return r


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_w4a8_decode_gemm_random(dt):
    """One decode shape per BM: more than one column tile with a ragged last one, K with a
    48-element tail after five whole k128 steps, and at BM = 16 more than one x panel (K = 2192:
    18 k128 steps)."""
    from lumen.ops.gemm import W4A8_BNS, w4a8_decode_gemm

    g = torch.Generator().manual_seed(23)
    for bm, M, K in ((16, 5, 2192), (64, 53, 688), (128, 128, 688), (256, 201, 688)):
        bn = W4A8_BNS[bm][-1]
        N = 2 * bn + 12
        xq, sx, w = rand_case(M, N, K, dt, g)
        for s in (1, 2):
            check(w4a8_decode_gemm(xq, sx, w, bm, bn, s), xq, sx, w, ("dgemm", bm, bn, M, K, s, dt))


def test_w4a8_decode_gemm_refusals():
    from lumen.ops._native import native

    g = torch.Generator().manual_seed(3)
    xq, sx, w = rand_case(17, 72, 400, torch.bfloat16, g)
    y = torch.empty(17, 72, device=DEV, dtype=torch.bfloat16)
    op = native().w4a8_decode_gemm
    with pytest.raises(Exception):                     # M above the block height
        op(xq, sx, w.q, w.scale, y, None, None, 16, 64, 1)
    with pytest.raises(Exception):                     # not a compiled variant
        op(xq, sx, w.q, w.scale, y, None, None, 64, 256, 1)
    with pytest.raises(Exception):                     # more slices than k128 steps
        op(xq, sx, w.q, w.scale, y, None, None, 64, 64, 5)
    with pytest.raises(Exception):                     # split-K without a workspace
        op(xq, sx, w.q, w.scale, y, None, None, 64, 64, 2)
    with pytest.raises(Exception):                     # scales of another K
        op(xq, sx, w.q, w.scale[:, :12].contiguous(), y, None, None, 64, 64, 1)
    with pytest.raises(Exception):                     # N % 4 != 0
        op(xq, sx, w.q[:70], w.scale[:70], y[:, :70], None, None, 64, 64, 1)


# ---- dispatch -----------------------------------------------------------------------------------

def test_linear_nt_dispatch(tmp_path, monkeypatch):
    """M = 1, 4, 16 always take the BM = 16 kernel (listed or not); a listed bucket takes the
    kernel; an unlisted bucket and M = 300 take the fallback; LUMEN_W8=0 forces the fallback.  The
    kernel within TOL of the definition, the fallback within 2 TOL (its extra 16-bit rounding)."""
    import lumen.ops.gemm as gm
    from lumen.ops.activation import swiglu
    from lumen.ops.quant import quantize_fp8_tokens, quantize_mxfp4_rows

    g = torch.Generator().manual_seed(11)
    N, K, dt = 1024, 688, torch.bfloat16
    path = tmp_path / "plans.json"
    path.write_text(json.dumps({"plans": [{"N": N, "K": K, "BM": 64, "BN": 128, "S": 2},
                                           {"N": N, "K": K, "BM": 256, "BN": 64, "S": 1}]}))
    monkeypatch.setenv("LUMEN_W4A8_PLANS", str(path))
    monkeypatch.setattr(gm, "_w4a8_plans", None)
    routes = []
    for name in ("w4a8_decode_gemm", "w4a8_fallback"):
        def wrap(*a, _f=getattr(gm, name), _n=name, **kw):
            routes.append((_n,) + tuple(a[3:6]))
            return _f(*a, **kw)
        monkeypatch.setattr(gm, name, wrap)
    w = quantize_mxfp4_rows((torch.randn(N, K, generator=g) * 0.02).to(DEV, dt))

    def run(x, on=True):
        monkeypatch.setattr(gm, "W8", on)
        routes.clear()
        y = gm.linear_nt(x, w)
        xq, sx = quantize_fp8_tokens(x)
        ref = (xq.double().cpu() @ wdq64(w).t()) * sx.double().cpu()[:, None]
        assert y.dtype == dt and y.shape == ref.shape
        return list(routes), rel(y.double().cpu(), ref)

    dflt = gm.w4a8_default_plan(N, K)
    want = {1: ("w4a8_decode_gemm", 16) + dflt, 4: ("w4a8_decode_gemm", 16) + dflt,
            16: ("w4a8_decode_gemm", 16) + dflt, 17: ("w4a8_decode_gemm", 64, 128, 2),
            100: ("w4a8_fallback",),               # the 128 bucket is not listed
            200: ("w4a8_decode_gemm", 256, 64, 1), 300: ("w4a8_fallback",)}
    for M, route in want.items():
        x = torch.randn(M, K, generator=g).to(DEV, dt)
        got, err = run(x)
        print("linear_nt", M, got, err)
        assert got == [route], (M, got)
        assert err < (2 if route[0] == "w4a8_fallback" else 1) * TOL[dt], (M, route, err)
        got, err = run(x, on=False)                     # LUMEN_W8=0
        assert got == [("w4a8_fallback",)] and err < 2 * TOL[dt], (M, got, err)
    # a view with a row stride the quant kernel refuses is copied, not refused
    xv = torch.randn(3, K + 4, generator=g).to(DEV, dt)[:, :K]
    got, err = run(xv)
    assert got[0][0] == "w4a8_decode_gemm" and err < TOL[dt]
    gu = torch.randn(3, 2 * K, generator=g).to(DEV, dt)
    assert torch.equal(gm.swiglu_linear_nt(gu, w), gm.linear_nt(swiglu(gu), w))


# ---- engine -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def served():
    m = ptpc_model(torch.bfloat16, DEV)
    return m, mxfp4_oracle(m), mxfp4_oracle(m, f32=True)


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("nprompts", [1, 3])
def test_engine_mxfp4_matches_fake_quant_oracle(served, nprompts, graphs):
    """1 / 3 concurrent prompts (the BM = 16 kernel at decode, the fallback at prefill), eager and
    graph-captured; the bound is tests/test_w8a8_gpu.py's: d = the oracle's own 16-bit noise,
    bound = max(3e-2, 2 d)."""
    m, oracle, oracle32 = served
    engine_checks(run_mxfp4_engine(m, oracle, oracle32, "cuda", nprompts, graphs),
                  ("engine", nprompts, graphs))


def test_engine_mxfp4_kernels_under_graph_capture(served, tmp_path, monkeypatch):
    """The shipped plan table lists no tiny-preset shape: a plan file forces the kernel on for all
    four projections (the down projection's K = 688 has a k tail) with split-K inside the captured
    decode graph, and on for the 128-token prefill chunks (BM = 128)."""
    import lumen.ops.gemm as gm

    shapes = {(512, 256), (256, 256), (1376, 256), (256, 688)}
    path = tmp_path / "plans.json"
    path.write_text(json.dumps({"plans": [
        {"N": n, "K": k, "BM": bm, "BN": 64, "S": 2 if k == 256 else 3}
        for n, k in shapes for bm in (16, 64, 128, 256)]}))
    monkeypatch.setenv("LUMEN_W4A8_PLANS", str(path))
    monkeypatch.setattr(gm, "_w4a8_plans", None)
    calls = []
    orig = gm.w4a8_decode_gemm

    def spy(xq, sx, w, bm, bn, s, out=None):
        calls.append((tuple(w.shape), xq.shape[0], bm, bn, s))
        return orig(xq, sx, w, bm, bn, s, out=out)
    monkeypatch.setattr(gm, "w4a8_decode_gemm", spy)
    m, oracle, oracle32 = served
    r = run_mxfp4_engine(m, oracle, oracle32, "cuda", 3, True, max_num_batched_tokens=128)
    assert {c[0] for c in calls} == shapes
    assert {c[2] for c in calls} == {16, 128}, {c[2] for c in calls}
    assert all(c[4] > 1 for c in calls) and gm._dg_ws
    for _, cnt in gm._dg_ws.values():            # every stream's tile counters are zero again
        assert int(cnt.abs().sum()) == 0
    engine_checks(r, ("engine, plan file", len(calls)))
