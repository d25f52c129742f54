"""fp8 activations x fp8 weights (--quantization ptpc_fp8) on the CPU: the per-token quantizer,
the torch reference path of ``linear_nt``, flags and the plan-table loader, and the engine end to
end against the fake-quant oracle.  The oracle and the engine harness below are shared with
tests/test_w8a8_gpu.py."""
import copy
import gc
import json

import pytest
import torch

from lumen.models import build_model
from lumen.serve.engine import EngineConfig, LLMEngine
from lumen.serve.model_runner import ServeWeights
from lumen.serve.sequence import SamplingParams
from tests.test_w8_gpu import PROMPTS   # plain data: importing it needs no GPU

PROJ = ("self_attn.qkv_proj", "self_attn.o_proj", "mlp.gate_up_proj", "mlp.down_proj")


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


# ---- the model and its fake-quant oracle (shared with the GPU tests) ----------------------------

def ptpc_model(dtype, device, seed=3):
    """tiny-llama-gqa whose greedy choices are decisive.  A random-init LM head gives near-uniform
    logits: the top-two margin of 512 Gaussian logits is ~1 % of the row's norm, far inside any
    quantization error bound, so no token could be checked.  Here the LM head row of token
    (7 t + 3) % V additionally carries 4 x the embedding of token t, and the two residual branches
    (o, down) are scaled by 1/4, so the model prefers "the successor of the current token" by a
    margin the projections still move (the bf16 oracle's own 16-bit noise d stays at 2.5-4 % of
    the logits).  Measured on the CPU with seed 3 in bf16, 1 / 3 / 7 prompts x 12 tokens: d =
    0.025 / 0.031 / 0.039, and the oracle's top-two margin exceeds 2 * max(3e-2, 2 d) * ||row||
    at every position (with the branches only halved, 36-45 % of the positions fall below it)."""
    m = build_model("tiny-llama-gqa", dtype=torch.float32, device="cpu", init="random", seed=seed)
    with torch.no_grad():
        V = m.lm_head.weight.shape[0]
        t = torch.arange(V)
        m.lm_head.weight[(7 * t + 3) % V] += 4.0 * m.embed_tokens.weight[t]
        for L in m.layers:
            L.self_attn.o_proj.weight.mul_(0.25)
            L.mlp.down_proj.weight.mul_(0.25)
    return m.to(device=device, dtype=dtype).eval()


def add_fake_quant_hooks(d):
    """Every projection input of ``d`` goes through ``quantize_fp8_tokens`` and back."""
    from lumen.ops.quant import quantize_fp8_tokens

    def hook(mod, args):
        x = args[0]
        xq, sx = quantize_fp8_tokens(x.reshape(-1, x.shape[-1]))
        return ((xq.float() * sx[:, None]).to(x.dtype).view(x.shape),) + tuple(args[1:])

    for L in d.layers:
        for name in PROJ:
            L.get_submodule(name).register_forward_pre_hook(hook)
    return d.eval()


def fake_quant_oracle(m, f32=False):
    """A deep copy of ``m`` whose four projection weights are replaced by their fp8 round trip
    (as test_w8_gpu.dequantized_copy) and whose projection inputs go through
    ``quantize_fp8_tokens`` and back (a forward pre-hook).  ``f32``: the same weights and the same
    fake-quant with f32 activations."""
    from lumen.ops.quant import quantize_fp8_rows

    d = copy.deepcopy(m)
    with torch.no_grad():
        for L in d.layers:
            for name in PROJ:
                lin = L.get_submodule(name)
                lin.weight.copy_(quantize_fp8_rows(lin.weight).dequant())
    return add_fake_quant_hooks(d.float() if f32 else d)


def run_ptpc_engine(m, oracle, oracle32, device, nprompts, graphs, max_tokens=12, **kw):
    """Serve ``nprompts`` prompts greedily with quantization="ptpc_fp8" and compare with the
    oracle's teacher-forced full forward.  Returns a dict:
    rels   per (decode step, row) relative error of the engine's logits row against the oracle's;
    d      the largest relative difference between the oracle in the model dtype and the oracle
           with f32 activations over those rows (the oracle's own 16-bit noise);
    bound  max(3e-2, 2 d);
    own    every sampled token attains the maximum of the engine's own logits row;
    agree, left_out   greedy agreement with the oracle's argmax over the positions whose top-two
           margin exceeds 2 * bound * ||row||, and the fraction of positions left out."""
    from lumen.ops.quant import QuantWeight

    dev = torch.device(device)
    eng = LLMEngine(EngineConfig(model="tiny-llama-gqa", device=device, max_model_len=512,
                                 block_size=16, num_blocks=128, use_graphs=graphs,
                                 quantization="ptpc_fp8", **kw), model=m)
    assert all(isinstance(w, QuantWeight) and w.act == "fp8" for L in eng.weights.layers
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
    if dev.type == "cuda":
        torch.cuda.synchronize()
    # the spy closes a reference cycle through the runner: undo it and free the engine (and its
    # captured graphs) here, not whenever the collector next runs (possibly inside a later
    # engine's graph capture)
    eng.runner.decode = orig
    del eng, orig, spy
    gc.collect()
    fulls = []
    for p, s in zip(prompts, seqs):
        assert len(s.output_ids) == max_tokens
        ids = torch.tensor([p + s.output_ids[:-1]], device=dev)
        with torch.no_grad():
            full = oracle(ids).float().view(ids.shape[1], -1)
            full32 = oracle32(ids).float().view(ids.shape[1], -1)
        fulls.append((p + s.output_ids, full, full32, len(p)))
    rels, ds, own = [], [], []
    for toks, pos, lg in got:
        toks, pos = toks.tolist(), pos.tolist()
        for i in range(min(len(toks), lg.shape[0])):
            # the row's sequence: the one holding this token at this position
            owners = [f for f in fulls if pos[i] < f[1].shape[0] and f[0][pos[i]] == toks[i]]
            if len(owners) == 1:
                ids, full, full32, _ = owners[0]
                rels.append(rel(lg[i], full[pos[i]]))
                ds.append(rel(full[pos[i]], full32[pos[i]]))
                own.append(bool(lg[i, ids[pos[i] + 1]] == lg[i].max()))
    d = max(ds)
    bound = max(3e-2, 2 * d)
    hit = counted = total = 0
    for ids, full, _, n in fulls:
        rows = full[n - 1:]
        top = rows.topk(2, dim=-1).values
        sure = (top[:, 0] - top[:, 1]) > 2 * bound * rows.norm(dim=-1)
        ref = rows.argmax(-1).tolist()
        for a, b, c in zip(ref, ids[n:], sure.tolist()):
            total += 1
            counted += int(c)
            hit += int(c and a == b)
    return {"rels": rels, "d": d, "bound": bound, "own": own, "agree": hit / max(counted, 1),
            "left_out": 1 - counted / total}


# ---- quantize_fp8_tokens ------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,K", [(1, 16), (5, 688), (67, 4112)])
def test_quantize_fp8_tokens(M, K, dt):
    from lumen.ops.quant import FP8_MAX, TINY, quantize_fp8_tokens

    g = torch.Generator().manual_seed(M * 31 + K)
    x = (torch.randn(M, K, generator=g) * torch.logspace(-3, 2, M)[:, None]).to(dt)
    xq, sx = quantize_fp8_tokens(x)
    assert xq.dtype == torch.float8_e4m3fn and xq.shape == (M, K) and xq.is_contiguous()
    assert sx.dtype == torch.float32 and sx.shape == (M,) and sx.is_contiguous()
    xf = x.float()
    amax = xf.abs().amax(1)
    want = torch.maximum(amax, torch.tensor(TINY, dtype=torch.float32)) / torch.tensor(
        FP8_MAX, dtype=torch.float32)
    assert want.dtype == torch.float32 and torch.equal(sx, want)
    qf = xq.float()
    assert not torch.isnan(qf).any()
    # the amax element becomes +-448
    idx = xf.abs().argmax(1)
    r = torch.arange(M)
    assert torch.equal(qf[r, idx], torch.sign(xf[r, idx]) * 448.0)
    # half an e4m3 ulp for normal values (3 mantissa bits: at most 1/17 < 2^-4 of the value) and
    # half the subnormal step (2^-9 in units of the scale)
    err = (qf * sx[:, None] - xf).abs()
    bound = xf.abs() * 2.0 ** -4 + sx[:, None] * 2.0 ** -10
    assert (err <= bound).all(), (err - bound).max().item()


def test_quantize_fp8_tokens_zero_row_and_max():
    from lumen.ops.quant import quantize_fp8_tokens

    g = torch.Generator().manual_seed(9)
    x = torch.randn(4, 64, generator=g).to(torch.float16)
    x[1] = 0
    x[2, 5] = 65504.0
    x[3, 7] = -65504.0
    xq, sx = quantize_fp8_tokens(x)
    byt = xq.view(torch.uint8)
    assert ((byt & 0x7F) != 0x7F).all()               # no NaN encoding
    assert torch.isfinite(sx).all() and (sx > 0).all()
    assert (xq.float()[1] == 0).all()
    assert xq.float()[2, 5] == 448.0 and xq.float()[3, 7] == -448.0
    xb = torch.randn(2, 32, generator=g).to(torch.bfloat16)
    xb[0, 3] = torch.finfo(torch.bfloat16).max
    qb, sb = quantize_fp8_tokens(xb)
    assert ((qb.view(torch.uint8) & 0x7F) != 0x7F).all() and torch.isfinite(sb).all()
    assert qb.float()[0, 3] == 448.0
    with pytest.raises(ValueError):
        quantize_fp8_tokens(torch.zeros(2, 3, 4))


# ---- linear_nt ----------------------------------------------------------------------------------

def test_linear_nt_cpu_is_the_definition():
    from lumen.ops.gemm import linear_nt, swiglu_linear_nt
    from lumen.ops.activation import swiglu
    from lumen.ops.quant import QuantWeight, quantize_fp8_rows, quantize_fp8_tokens

    g = torch.Generator().manual_seed(5)
    for dt, tol in ((torch.float32, 1e-6), (torch.bfloat16, 2.0 ** -8)):
        w = (torch.randn(68, 688, generator=g) * 0.02).to(dt)
        qw = quantize_fp8_rows(w)
        assert qw.act is None
        qa = QuantWeight(qw.q, qw.scale, qw.dtype, act="fp8")
        x = torch.randn(7, 688, generator=g).to(dt)
        xq, sx = quantize_fp8_tokens(x)
        ref = (xq.double() @ qw.q.double().t()) * sx.double()[:, None] * qw.scale.double()[None, :]
        y = linear_nt(x, qa)
        assert y.shape == (7, 68) and y.dtype == dt
        assert rel(y, ref) < tol
        # not the weight-only function: the activations really were quantized
        assert rel(linear_nt(x, qw), ref) > 1e-3
        gu = torch.randn(3, 2 * 688, generator=g).to(dt)
        assert torch.equal(swiglu_linear_nt(gu, qa), linear_nt(swiglu(gu), qa))
    with pytest.raises(ValueError):
        linear_nt(x, QuantWeight(qw.q, qw.scale, qw.dtype, act="int8"))


# ---- flags, config, plan table --------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    return ptpc_model(torch.float32, "cpu")


def test_serve_weights_and_config_accept_ptpc_fp8(model):
    from lumen.ops.quant import QuantWeight, quantize_fp8_rows

    plain = ServeWeights(model, 0, 1)
    w = ServeWeights(model, 0, 1, "ptpc_fp8")
    assert w.quantization == "ptpc_fp8"
    for Lp, Lq in zip(plain.layers, w.layers):
        for name in ("qkv", "o", "gate_up", "down"):
            qw, ref = getattr(Lq, name), quantize_fp8_rows(getattr(Lp, name))
            assert isinstance(qw, QuantWeight) and qw.act == "fp8"
            assert torch.equal(qw.q.view(torch.uint8), ref.q.view(torch.uint8))
            assert torch.equal(qw.scale, ref.scale)
    assert all(getattr(L, n).act is None for L in ServeWeights(model, 0, 1, "fp8").layers
               for n in ("qkv", "o", "gate_up", "down"))
    assert not isinstance(w.lm_head, QuantWeight)
    with pytest.raises(ValueError):
        ServeWeights(model, 0, 1, "ptpc_fp4")
    with pytest.raises(ValueError):
        LLMEngine(EngineConfig(model="tiny-llama-gqa", device="cpu", max_model_len=64,
                               block_size=4, use_graphs=False, num_blocks=32,
                               quantization="ptpc_fp4"), model=model)
    eng = LLMEngine(EngineConfig(model="tiny-llama-gqa", device="cpu", max_model_len=64,
                                 block_size=4, use_graphs=False, num_blocks=32,
                                 quantization="ptpc_fp8"), model=model)
    assert eng.weights.quantization == "ptpc_fp8"


def test_tp_rank_quantizes_its_own_slice():
    from lumen.ops.quant import quantize_fp8_rows

    m = build_model("tiny-llama-tp8", dtype=torch.bfloat16, device="cpu", init="random", seed=2)
    m.eval()
    for r in (0, 1):
        plain, quant = ServeWeights(m, r, 2), ServeWeights(m, r, 2, "ptpc_fp8")
        for Lp, Lq in zip(plain.layers, quant.layers):
            for name in ("qkv", "o", "gate_up", "down"):
                qw, ref = getattr(Lq, name), quantize_fp8_rows(getattr(Lp, name))
                assert qw.act == "fp8" and tuple(qw.shape) == tuple(ref.shape)
                assert torch.equal(qw.q.view(torch.uint8), ref.q.view(torch.uint8)), (r, name)


def test_cli_and_bench_accept_the_flag():
    from lumen.cli.serve import build_parser

    p = build_parser()
    assert p.parse_args(["--model", "tiny-llama", "--quantization", "ptpc_fp8"]
                        ).quantization == "ptpc_fp8"
    assert p.parse_args(["--model", "tiny-llama", "--quantization", "fp8"]).quantization == "fp8"
    with pytest.raises(SystemExit):
        p.parse_args(["--model", "tiny-llama", "--quantization", "ptpc"])


def test_plan_table_loader(tmp_path, monkeypatch):
    import lumen.ops.gemm as gm

    path = tmp_path / "plans.json"
    path.write_text(json.dumps({"plans": [
        {"N": 12288, "K": 4096, "BM": 64, "BN": 64, "S": 2},
        {"N": 4096, "K": 11008, "BM": 256, "BN": 64, "S": 3, "us": 55.0},
        {"N": 4096, "K": 4096, "BM": 2048, "BN": 128, "S": 1}]}))
    want = {(12288, 4096, 64): (64, 2), (4096, 11008, 256): (64, 3), (4096, 4096, 2048): (128, 1)}
    assert gm.load_w8a8_plans(str(path)) == want
    assert gm.load_w8a8_plans(str(tmp_path / "missing.json")) == {}
    monkeypatch.setenv("LUMEN_W8A8_PLANS", str(path))
    monkeypatch.setattr(gm, "_w8a8_plans", None)
    assert gm.w8a8_plans() == want
    # the shipped table lists compiled variants and known buckets only
    monkeypatch.delenv("LUMEN_W8A8_PLANS")
    monkeypatch.setattr(gm, "_w8a8_plans", None)
    for (N, K, bm), (bn, s) in gm.w8a8_plans().items():
        if bm <= 256:
            assert bm in gm.W8A8_BNS and bn in gm.W8A8_BNS[bm] and 1 <= s <= -(-K // 128)
        else:
            assert bm in gm.W8A8_GEMM_BUCKETS and (128, bn) in gm.W8A8_GEMM_TILES and s == 1
        assert K % 16 == 0 and N % 4 == 0
    assert gm.w8a8_gemm_bucket(257) == 512 and gm.w8a8_gemm_bucket(2048) == 2048
    assert gm.w8a8_gemm_bucket(10 ** 6) == gm.W8A8_GEMM_BUCKETS[-1]


# ---- engine -------------------------------------------------------------------------------------

def test_engine_cpu_ptpc_fp8_matches_fake_quant_oracle(model):
    before = {n: p.clone() for n, p in model.named_parameters()}
    oracle = fake_quant_oracle(model)
    r = run_ptpc_engine(model, oracle, oracle, "cpu", 3, False)
    for n, p in model.named_parameters():       # a model passed in by the caller is left untouched
        assert torch.equal(p, before[n]), n
    print("d", r["d"], "bound", r["bound"], "max logits rel", max(r["rels"]), "rows",
          len(r["rels"]), "agreement", r["agree"], "left out", r["left_out"])
    assert len(r["rels"]) >= 10
    assert r["d"] == 0.0 and r["bound"] == 3e-2        # both oracles are f32 here
    assert max(r["rels"]) < r["bound"], max(r["rels"])
    assert all(r["own"])
    assert r["left_out"] <= 0.25, r["left_out"]
    assert r["agree"] >= 0.9, r["agree"]
