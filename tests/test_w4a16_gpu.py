"""MXFP4 weight-only quantization (--quantization mxfp4_a16) on the GPU: kernels/w4a16_gemm.hip's
GEMV and MFMA kernel on exact data (which fixes the lane-to-k maps and the scale lane map) and on
random data against the f64 definition, their refusals, the ``linear_nt`` dispatch, and the engine
against the dequantised-weight oracle of tests/test_w4a16_cpu.py."""
import json

import pytest
import torch

from tests.test_mxfp4_gpu import holder, wdq64
from tests.test_w4a16_cpu import engine_checks, run_w4a16_engine, w4a16_oracle
from tests.test_w8a8_cpu import ptpc_model, rel
from tests.test_w8a8_gpu import TOL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
# (72, 400): 13 blocks, fewer than the lanes, a partial last block; (1032, 256): below one wave
# step; (68, 8720): five 2048-k steps over two waves with a ragged tail, N % 8 != 0; (20, 6160):
# four steps, one per wave (the four-wave split), the last ragged, and a last workgroup with four
# of its eight rows
GEMV_SHAPES = [(72, 400), (1032, 256), (68, 8720), (20, 6160)]


def weight_only(w):
    w.act = None
    return w


def wide(t, pad, fill):
    """``t`` as a view of a buffer ``pad`` columns wider, the extra columns holding ``fill``."""
    b = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device=t.device)
    b[:, :t.shape[1]] = t
    return b[:, :t.shape[1]]


_ints = {}


def int_case(M, N, K, dt):
    """tests/test_mxfp4_gpu.int_case's integer formulas for the codes and the block exponents
    (exponents in {-1, 0, 1, 2}: 4 * wdq is an integer of magnitude <= 96) and x = integers in
    [-8, 8] times 2^-4 by a different formula of (m, k), exact in bf16 and fp16.  64 * sum_k |x w|
    is an integer below 2^24 (asserted), so every partial sum in every order is exact in f32 and y
    must EQUAL the f64 reference rounded once."""
    if (M, N, K) not in _ints:
        n, k = torch.arange(N)[:, None], torch.arange(-(-K // 32) * 32)[None, :]
        m, b = torch.arange(M)[:, None], torch.arange(-(-K // 32))[None, :]
        codes = (5 * n + 3 * k + (n * k) // 7 + 1) % 16
        e = (3 * n + 2 * b + (n * b) // 5) % 4 - 1
        xi = (3 * m + 5 * k[:, :K] + m * k[:, :K]) % 17 - 8
        _ints[(M, N, K)] = (codes, e + 127, xi.double() / 16)
    codes, eb, x = _ints[(M, N, K)]
    w = weight_only(holder(codes, eb, K, dt))
    wd = wdq64(w)
    acc = x @ wd.t()
    assert (64 * acc == (64 * acc).round()).all()
    assert 64 * (x.abs() @ wd.abs().t()).max() < 2 ** 24
    xg = x.to(dt).to(DEV)
    assert torch.equal(xg.double().cpu(), x)
    return xg, w, acc.to(dt).to(DEV)


# ---- the GEMV -----------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K", GEMV_SHAPES)
def test_w4a16_gemv_exact(N, K):
    """M = 1 .. 4, both types, the default and every compiled (R, GS); x rows in a wider buffer
    whose padding is NaN (a read past K would show), y inside a wider buffer whose sentinel rows
    and columns survive."""
    from lumen.ops.gemm import W4A16_GEMV_CFGS, w4a16_gemv

    for dt in (torch.bfloat16, torch.float16):
        for M in (1, 2, 3, 4):
            x, w, ref = int_case(M, N, K, dt)
            xv = wide(x, 24, float("nan"))
            for cfg in (0,) + W4A16_GEMV_CFGS:
                if cfg == 82 and M > 2:
                    continue            # not compiled (refused: test_refusals)
                yb = torch.full((M + 1, N + 8), 777.0, device=DEV, dtype=dt)
                w4a16_gemv(xv, w, out=yb[:M, :N], cfg=cfg)
                assert torch.equal(yb[:M, :N], ref), ("exact", N, K, M, cfg, dt)
                assert (yb[:, N:] == 777.0).all() and (yb[M:] == 777.0).all()


def rand_case(M, N, K, dt, g):
    """Random codes and scale bytes 2^-10 .. 2^-4 (tests/test_mxfp4_gpu.rand_case's), Gaussian x;
    in fp16 x is scaled so that |y| < 3e4."""
    Kp = -(-K // 32) * 32
    w = weight_only(holder(torch.randint(0, 16, (N, Kp), generator=g),
                           torch.randint(117, 124, (N, Kp // 32), generator=g), K, dt))
    x = torch.randn(M, K, generator=g).to(dt)
    if dt == torch.float16:
        top = (x.double() @ wdq64(w).t()).abs().max()
        x = (x.double() * min(1.0, 3e4 / top)).to(dt)
    return x.to(DEV), w


def check(y, x, w, what, tol=1.0):
    """The product against the definition formed in f64 (the weights are exact in both types
    here): the same accumulation and the same single output rounding."""
    ref = x.double().cpu() @ wdq64(w).t()
    assert y.shape == ref.shape and y.dtype == w.dtype, what
    assert w.dtype != torch.float16 or ref.abs().max() < 3e4, what
    r = rel(y.double().cpu(), ref)
    print(what, "rel", r)
    assert r < tol * TOL[w.dtype], (what, r)
    return r


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_w4a16_gemv_random(dt):
    from lumen.ops.gemm import w4a16_gemv

    g = torch.Generator().manual_seed(29)
    for N, K in GEMV_SHAPES:
        for M in (1, 2, 3, 4):
            x, w = rand_case(M, N, K, dt, g)
            check(w4a16_gemv(wide(x, 8, 1.0), w), x, w, ("gemv", N, K, M, dt))


# ---- the MFMA kernel ----------------------------------------------------------------------------

@pytest.mark.parametrize("bm", [64, 128, 256])
def test_w4a16_decode_gemm_exact(bm):
    """Every compiled (BM, BN) at every M <= BM of the list, split-K 1 and 3, N = 72 (a partial
    16-row tile, not a multiple of any BN), K = 416 = 13 blocks (six k64 stages and half a
    stage); the output buffer is wider than N and its sentinel survives; the tile counters are
    zero after every split-K launch."""
    from lumen.ops.gemm import W4A16_BNS, dg_workspace, w4a16_decode_gemm

    for dt in (torch.bfloat16, torch.float16):
        for M in (m for m in (5, 16, 17, 64, 200) if m <= bm):
            x, w, ref = int_case(M, 72, 416, dt)
            xv = wide(x, 24, float("nan"))
            for bn in W4A16_BNS[bm]:
                for s in (1, 3):
                    yb = torch.full((M + 1, 72 + 8), 777.0, device=DEV, dtype=dt)
                    w4a16_decode_gemm(xv, w, bm, bn, s, out=yb[:M, :72])
                    assert torch.equal(yb[:M, :72], ref), ("exact", bm, bn, M, s, dt)
                    assert (yb[:, 72:] == 777.0).all() and (yb[M:] == 777.0).all()
                    if s > 1:
                        assert int(dg_workspace(DEV)[1].abs().sum()) == 0


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_w4a16_decode_gemm_random(dt):
    """One decode shape per BM: more than one column tile with a ragged last one, K = 672 = 21
    blocks (ten k64 stages and half a stage)."""
    from lumen.ops.gemm import W4A16_BNS, w4a16_decode_gemm

    g = torch.Generator().manual_seed(31)
    for bm, M in ((64, 53), (128, 128), (256, 201)):
        bn = W4A16_BNS[bm][-1]
        N = 2 * bn + 12
        x, w = rand_case(M, N, 672, dt, g)
        for s in (1, 2):
            check(w4a16_decode_gemm(x, w, bm, bn, s), x, w, ("dgemm", bm, bn, M, s, dt))


def test_refusals():
    from lumen.ops._native import native

    g = torch.Generator().manual_seed(3)
    dt = torch.bfloat16
    x, w = rand_case(17, 72, 416, dt, g)
    y = torch.empty(17, 72, device=DEV, dtype=dt)
    gemv, op = native().w4a16_gemv, native().w4a16_decode_gemm
    with pytest.raises(Exception):                     # the GEMV stops at M = 4
        gemv(x[:5], w.q, w.scale, y[:5], 0)
    with pytest.raises(Exception):                     # an x row stride that is no multiple of 8
        gemv(wide(x[:2], 4, 0.0), w.q, w.scale, y[:2], 0)
    with pytest.raises(Exception):                     # not a compiled (R, GS)
        gemv(x[:2], w.q, w.scale, y[:2], 43)
    with pytest.raises(Exception):                     # (R, GS) = (8, 2) is not compiled for M > 2
        gemv(x[:3], w.q, w.scale, y[:3], 82)
    with pytest.raises(Exception):                     # scales of another K
        gemv(x[:2], w.q, w.scale[:, :12].contiguous(), y[:2], 0)
    with pytest.raises(Exception):                     # N % 4 != 0
        gemv(x[:2], w.q[:70], w.scale[:70], y[:2, :70], 0)
    gemv(x[:2], w.q, w.scale, y[:2], 0)                # the arguments above are otherwise fine
    with pytest.raises(Exception):                     # M above the block height
        op(x.repeat(4, 1), w.q, w.scale, y.repeat(4, 1), None, None, 64, 64, 1)
    with pytest.raises(Exception):                     # not a compiled variant
        op(x, w.q, w.scale, y, None, None, 64, 256, 1)
    with pytest.raises(Exception):                     # more slices than k64 stages
        op(x, w.q, w.scale, y, None, None, 64, 64, 8)
    with pytest.raises(Exception):                     # split-K without a workspace
        op(x, w.q, w.scale, y, None, None, 64, 64, 2)
    with pytest.raises(Exception):                     # scales of another K
        op(x, w.q, w.scale[:, :12].contiguous(), y, None, None, 64, 64, 1)
    with pytest.raises(Exception):                     # N % 4 != 0
        op(x, w.q[:70], w.scale[:70], y[:, :70], None, None, 64, 64, 1)
    x2, w2 = rand_case(17, 72, 400, dt, g)             # K % 32 != 0: the GEMV takes it, this not
    with pytest.raises(Exception):
        op(x2, w2.q, w2.scale, y, None, None, 64, 64, 1)
    op(x, w.q, w.scale, y, None, None, 64, 64, 1)      # and the arguments are otherwise fine
    torch.cuda.synchronize()


# ---- dispatch -----------------------------------------------------------------------------------

def test_linear_nt_dispatch(tmp_path, monkeypatch):
    """M = 3 takes the GEMV; M = 40 the MFMA kernel when its bucket is listed and the fallback when
    it is not; M = 300 the fallback; LUMEN_W8=0 the fallback at M = 1; an ``act="fp8"`` holder
    still takes the W4A8 route.  Every route within TOL of the definition."""
    import lumen.ops.gemm as gm
    from lumen.ops.activation import swiglu
    from lumen.ops.quant import quantize_mxfp4_rows

    g = torch.Generator().manual_seed(11)
    N, K, dt = 1024, 672, torch.bfloat16
    path = tmp_path / "plans.json"
    path.write_text(json.dumps({"plans": [{"N": N, "K": K, "BM": 64, "BN": 128, "S": 2}]}))
    monkeypatch.setenv("LUMEN_W4A16_PLANS", str(path))
    monkeypatch.setattr(gm, "_w4a16_plans", None)
    routes = []
    for name in ("w4a16_gemv", "w4a16_decode_gemm", "w4a16_fallback", "w4a8_decode_gemm"):
        def wrap(*a, _f=getattr(gm, name), _n=name, **kw):
            routes.append((_n,) + tuple(a[2:5]) if _n == "w4a16_decode_gemm" else (_n,))
            return _f(*a, **kw)
        monkeypatch.setattr(gm, name, wrap)
    w8 = quantize_mxfp4_rows((torch.randn(N, K, generator=g) * 0.02).to(DEV, dt))
    w = weight_only(quantize_mxfp4_rows(w8.dequant()))

    def run(x, on=True):
        monkeypatch.setattr(gm, "W8", on)
        routes.clear()
        y = gm.linear_nt(x, w)
        monkeypatch.setattr(gm, "W8", True)
        check(y, x, w, ("linear_nt", x.shape[0], on))
        return list(routes)

    xs = {M: torch.randn(M, K, generator=g).to(DEV, dt) for M in (1, 3, 40, 100, 300)}
    assert run(xs[3]) == [("w4a16_gemv",)]
    assert run(xs[40]) == [("w4a16_decode_gemm", 64, 128, 2)]
    assert run(xs[100]) == [("w4a16_fallback",)]        # the 128 bucket is not listed
    assert run(xs[300]) == [("w4a16_fallback",)]
    assert run(xs[1]) == [("w4a16_gemv",)]
    assert run(xs[1], on=False) == [("w4a16_fallback",)]
    assert run(xs[40], on=False) == [("w4a16_fallback",)]
    monkeypatch.setattr(gm, "_w4a16_plans", {})
    assert run(xs[40]) == [("w4a16_fallback",)]         # no longer listed
    # a view the GEMV refuses (row stride % 8 != 0) takes the fallback, not an error
    assert run(wide(xs[3], 4, 0.0)) == [("w4a16_fallback",)]
    gu = torch.randn(3, 2 * K, generator=g).to(DEV, dt)
    assert torch.equal(gm.swiglu_linear_nt(gu, w), gm.linear_nt(swiglu(gu), w))
    routes.clear()
    gm.linear_nt(xs[3], w8)
    assert [r[0] for r in routes] == ["w4a8_decode_gemm"]
    monkeypatch.setattr(gm, "_w4a16_plans", None)


# ---- engine -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def served():
    m = ptpc_model(torch.bfloat16, DEV)
    return m, w4a16_oracle(m), w4a16_oracle(m, f32=True)


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("nprompts", [1, 3, 7])
def test_engine_mxfp4_a16_matches_dequantised_oracle(served, nprompts, graphs):
    """1 / 3 / 7 concurrent prompts (the GEMV at decode up to 4 rows, the fallback above and at
    prefill), eager and graph-captured; d = the oracle's own bf16-against-f32 noise, bound =
    max(3e-2, 2 d).  Measured on an MI355X (profiles/w4a16_serve/README.md)."""
    m, oracle, oracle32 = served
    engine_checks(run_w4a16_engine(m, oracle, oracle32, "cuda", nprompts, graphs),
                  ("engine", nprompts, graphs))


def test_engine_mxfp4_a16_mfma_under_graph_capture(served, tmp_path, monkeypatch):
    """The shipped plan table lists no tiny-preset shape: a plan file lists all four projections
    with and without split-K, and 7 prompts decode on the MFMA kernel inside the captured graph
    (3 prompts: on the GEMV) while the 128-token prefill chunks take BM = 128.  The down
    projection's K = 688 is no whole number of blocks: the MFMA kernel does not apply there and it
    takes the fallback."""
    import lumen.ops.gemm as gm

    shapes = {(512, 256): 2, (256, 256): 1, (1376, 256): 4, (256, 688): 3}
    path = tmp_path / "plans.json"
    path.write_text(json.dumps({"plans": [
        {"N": n, "K": k, "BM": bm, "BN": 64, "S": s}
        for (n, k), s in shapes.items() for bm in (64, 128, 256)]}))
    monkeypatch.setenv("LUMEN_W4A16_PLANS", str(path))
    monkeypatch.setattr(gm, "_w4a16_plans", None)
    calls = []
    orig = gm.w4a16_decode_gemm

    def spy(x, w, bm, bn, s, out=None):
        calls.append((tuple(w.shape), x.shape[0], bm, bn, s))
        return orig(x, w, bm, bn, s, out=out)
    monkeypatch.setattr(gm, "w4a16_decode_gemm", spy)
    m, oracle, oracle32 = served
    for nprompts in (3, 7):
        calls.clear()
        r = run_w4a16_engine(m, oracle, oracle32, "cuda", nprompts, True,
                             max_num_batched_tokens=128)
        assert {c[0] for c in calls} == {sh for sh in shapes if sh[1] % 32 == 0}
        assert {c[4] for c in calls} == {1, 2, 4} and gm._dg_ws
        assert {c[2] for c in calls} <= {64, 128} and all(c[1] > 4 for c in calls)
        # the captured decode graph pads 7 rows to 8; the other calls are prefill chunks
        assert any(c[1] <= 8 for c in calls) == (nprompts == 7), {c[1:3] for c in calls}
        for _, cnt in gm._dg_ws.values():        # every stream's tile counters are zero again
            assert int(cnt.abs().sum()) == 0
        engine_checks(r, ("engine, plan file", nprompts, len(calls)))
    monkeypatch.setattr(gm, "_w4a16_plans", None)
