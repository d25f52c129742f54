"""MXFP4 weight-only quantization (--quantization mxfp4_a16) on the CPU: the ``act`` field of the
holder and the torch definition behind ``linear_nt``, flags, TP slicing and the plan-table loader,
and the engine end to end against a model whose projection weights are the dequantised MXFP4
weights.  The oracle and the engine harness below are shared with tests/test_w4a16_gpu.py."""
import copy
import gc
import json

import pytest
import torch

from lumen.models import build_model
from lumen.serve.engine import EngineConfig, LLMEngine
from lumen.serve.model_runner import ServeWeights
from lumen.serve.sequence import SamplingParams
from tests.test_mxfp4_cpu import NAMES, PROJ
from tests.test_w8a8_cpu import PROMPTS, ptpc_model, rel


# ---- the oracle and the engine harness (shared with the GPU tests) ------------------------------

def w4a16_oracle(m, f32=False):
    """A deep copy of ``m`` whose four projection weights are replaced by
    ``quantize_mxfp4_rows(w).dequant()``; the activations are left alone.  ``f32``: the same
    weights with f32 activations."""
    from lumen.ops.quant import quantize_mxfp4_rows

    d = copy.deepcopy(m)
    with torch.no_grad():
        for L in d.layers:
            for name in PROJ:
                lin = L.get_submodule(name)
                lin.weight.copy_(quantize_mxfp4_rows(lin.weight).dequant())
    return (d.float() if f32 else d).eval()


def run_w4a16_engine(m, oracle, oracle32, device, nprompts, graphs, max_tokens=12, **kw):
    """tests/test_mxfp4_cpu.run_mxfp4_engine with quantization="mxfp4_a16": serve ``nprompts``
    prompts greedily, spy on ``runner.decode`` and compare every row with the oracle's
    teacher-forced full forward.  Returns that harness's dict (rels, d, bound = max(3e-2, 2 d),
    own, agree, left_out) plus ``same``: whether every served token is the oracle's argmax."""
    from lumen.ops.quant import Mxfp4Weight

    dev = torch.device(device)
    eng = LLMEngine(EngineConfig(model="tiny-llama-gqa", device=device, max_model_len=512,
                                 block_size=16, num_blocks=128, use_graphs=graphs,
                                 quantization="mxfp4_a16", **kw), model=m)
    assert all(isinstance(getattr(L, n), Mxfp4Weight) and getattr(L, n).act is None
               for L in eng.weights.layers for n in NAMES)
    assert isinstance(eng.weights.lm_head, torch.Tensor)
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
    # undo the reference cycle through the runner and free the engine (and its captured graphs)
    # here, not whenever the collector next runs (possibly inside a later engine's graph capture)
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
            owners = [f for f in fulls if pos[i] < f[1].shape[0] and f[0][pos[i]] == toks[i]]
            if len(owners) == 1:
                ids, full, full32, _ = owners[0]
                rels.append(rel(lg[i], full[pos[i]]))
                ds.append(rel(full[pos[i]], full32[pos[i]]))
                own.append(bool(lg[i, ids[pos[i] + 1]] == lg[i].max()))
    d = max(ds)
    bound = max(3e-2, 2 * d)
    hit = counted = total = same = 0
    for ids, full, _, n in fulls:
        rows = full[n - 1:]
        top = rows.topk(2, dim=-1).values
        sure = (top[:, 0] - top[:, 1]) > 2 * bound * rows.norm(dim=-1)
        ref = rows.argmax(-1).tolist()
        for a, b, c in zip(ref, ids[n:], sure.tolist()):
            total += 1
            counted += int(c)
            hit += int(c and a == b)
            same += int(a == b)
    return {"rels": rels, "d": d, "bound": bound, "own": own, "agree": hit / max(counted, 1),
            "left_out": 1 - counted / total, "same": same == total}


def engine_checks(r, what):
    print(what, "d", r["d"], "bound", r["bound"], "max logits rel", max(r["rels"]), "rows",
          len(r["rels"]), "agreement", r["agree"], "left out", r["left_out"])
    assert len(r["rels"]) >= 10
    assert max(r["rels"]) < r["bound"], (max(r["rels"]), r["bound"])
    assert all(r["own"])
    assert r["agree"] >= 0.9, r["agree"]
    assert r["left_out"] <= 0.25, r["left_out"]


# ---- the holder and linear_nt -------------------------------------------------------------------

def test_act_defaults_to_fp8_and_keeps_the_w4a8_function():
    from lumen.ops.gemm import linear_nt
    from lumen.ops.quant import Mxfp4Weight, quantize_fp8_tokens, quantize_mxfp4_rows

    g = torch.Generator().manual_seed(5)
    w = (torch.randn(68, 400, generator=g) * 0.02)
    qw = quantize_mxfp4_rows(w)
    assert qw.act == "fp8"
    assert Mxfp4Weight(qw.q, qw.scale, 400, torch.float32).act == "fp8"
    x = torch.randn(7, 400, generator=g)
    xq, sx = quantize_fp8_tokens(x)
    want = ((xq.float() @ qw.dequant_f32().t()) * sx[:, None]).to(x.dtype)
    assert torch.equal(linear_nt(x, qw), want)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_linear_nt_cpu_is_the_definition(dt):
    from lumen.ops.activation import swiglu
    from lumen.ops.gemm import linear_nt, swiglu_linear_nt
    from lumen.ops.quant import Mxfp4Weight, quantize_mxfp4_rows

    g = torch.Generator().manual_seed(6)
    w = (torch.randn(68, 400, generator=g) * 0.02).to(dt)       # K = 400: a partial last block
    q8 = quantize_mxfp4_rows(w)
    qw = Mxfp4Weight(q8.q, q8.scale, 400, dt, act=None)
    assert qw.act is None and torch.equal(qw.dequant(), q8.dequant())
    for M in (7, 1, 0):
        x = torch.randn(M, 400, generator=g).to(dt)
        want = (x.float() @ qw.dequant().float().t()).to(dt)
        y = linear_nt(x, qw)
        assert y.shape == (M, 68) and y.dtype == dt and torch.equal(y, want)
        if M == 7:      # not the W4A8 function of the same inputs
            assert not torch.equal(linear_nt(x, q8), y)
    gu = torch.randn(3, 800, generator=g).to(dt)
    assert torch.equal(swiglu_linear_nt(gu, qw), linear_nt(swiglu(gu), qw))
    with pytest.raises(ValueError, match="act"):
        linear_nt(torch.randn(2, 400).to(dt), Mxfp4Weight(q8.q, q8.scale, 400, dt, act="int8"))


# ---- flags, config, TP, plan table ----------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    return ptpc_model(torch.float32, "cpu")


def test_serve_weights_and_config_accept_mxfp4_a16(model):
    from lumen.ops.quant import Mxfp4Weight, quantize_mxfp4_rows

    plain = ServeWeights(model, 0, 1)
    w = ServeWeights(model, 0, 1, "mxfp4_a16")
    assert w.quantization == "mxfp4_a16"
    for Lp, Lq in zip(plain.layers, w.layers):
        for name in NAMES:
            qw, ref = getattr(Lq, name), quantize_mxfp4_rows(getattr(Lp, name))
            assert isinstance(qw, Mxfp4Weight) and qw.act is None
            assert tuple(qw.shape) == tuple(getattr(Lp, name).shape)
            assert torch.equal(qw.q, ref.q) and torch.equal(qw.scale, ref.scale)
    assert isinstance(w.lm_head, torch.Tensor) and torch.equal(w.lm_head, plain.lm_head)
    # "mxfp4" still means W4A8
    assert all(getattr(L, n).act == "fp8" for L in ServeWeights(model, 0, 1, "mxfp4").layers
               for n in NAMES)
    kw = dict(model="tiny-llama-gqa", device="cpu", max_model_len=64, block_size=4,
              use_graphs=False, num_blocks=32)
    with pytest.raises(ValueError, match="mxfp4_a16"):
        ServeWeights(model, 0, 1, "int3")
    with pytest.raises(ValueError, match="mxfp4_a16"):
        LLMEngine(EngineConfig(quantization="int3", **kw), model=model)
    eng = LLMEngine(EngineConfig(quantization="mxfp4_a16", **kw), model=model)
    assert eng.weights.quantization == "mxfp4_a16"


def test_tp_rank_quantizes_its_own_slice():
    from lumen.ops.quant import quantize_mxfp4_rows

    m = build_model("tiny-llama-tp8", dtype=torch.bfloat16, device="cpu", init="random", seed=2)
    m.eval()
    for r in (0, 1):
        plain, quant = ServeWeights(m, r, 2), ServeWeights(m, r, 2, "mxfp4_a16")
        for Lp, Lq in zip(plain.layers, quant.layers):
            for name in NAMES:
                qw, ref = getattr(Lq, name), quantize_mxfp4_rows(getattr(Lp, name))
                assert qw.act is None
                assert tuple(qw.shape) == tuple(ref.shape) == tuple(getattr(Lp, name).shape)
                assert torch.equal(qw.q, ref.q) and torch.equal(qw.scale, ref.scale), (r, name)


def test_cli_and_bench_accept_the_flag(monkeypatch):
    import sys

    from lumen.bench import serve_bench
    from lumen.cli.serve import build_parser

    p = build_parser()
    assert p.parse_args(["--model", "tiny-llama", "--quantization", "mxfp4_a16"]
                        ).quantization == "mxfp4_a16"
    with pytest.raises(SystemExit):
        p.parse_args(["--model", "tiny-llama", "--quantization", "int3"])
    # serve_bench parses in main(): stop it where it would build the engine
    seen = []

    class Stop(Exception):
        pass

    def make_engine(a):
        seen.append(a.quantization)
        raise Stop

    monkeypatch.setattr(serve_bench, "make_engine", make_engine)
    monkeypatch.setattr(sys, "argv", ["serve_bench", "--quantization", "mxfp4_a16"])
    with pytest.raises(Stop):
        serve_bench.main()
    assert seen == ["mxfp4_a16"]
    monkeypatch.setattr(sys, "argv", ["serve_bench", "--quantization", "int3"])
    with pytest.raises(SystemExit):
        serve_bench.main()


def test_plan_table_loader(tmp_path, monkeypatch):
    import lumen.ops.gemm as gm

    path = tmp_path / "plans.json"
    path.write_text(json.dumps({"plans": [
        {"N": 12288, "K": 4096, "BM": 64, "BN": 128, "S": 2},
        {"N": 4096, "K": 11008, "BM": 256, "BN": 64, "S": 3, "us": 55.0}]}))
    want = {(12288, 4096, 64): (128, 2), (4096, 11008, 256): (64, 3)}
    assert gm.load_w4a16_plans(str(path)) == want
    assert gm.load_w4a16_plans(str(tmp_path / "missing.json")) == {}
    monkeypatch.setenv("LUMEN_W4A16_PLANS", str(path))
    monkeypatch.setattr(gm, "_w4a16_plans", None)
    assert gm.w4a16_plans() == want
    monkeypatch.setenv("LUMEN_W4A16_PLANS", str(tmp_path / "missing.json"))
    monkeypatch.setattr(gm, "_w4a16_plans", None)
    assert gm.w4a16_plans() == {}
    # the shipped table parses and lists compiled variants only
    monkeypatch.delenv("LUMEN_W4A16_PLANS")
    monkeypatch.setattr(gm, "_w4a16_plans", None)
    for (N, K, bm), (bn, s) in gm.w4a16_plans().items():
        assert bm in gm.W4A16_BNS and bn in gm.W4A16_BNS[bm] and 1 <= s <= -(-K // 64)
        assert K % 32 == 0 and N % 4 == 0
    assert set(gm.W4A16_BNS) == set(gm.W4A16_BMS) == {64, 128, 256}
    monkeypatch.setattr(gm, "_w4a16_plans", None)


# ---- engine -------------------------------------------------------------------------------------

def test_engine_cpu_mxfp4_a16_matches_dequantised_oracle(model):
    before = {n: p.clone() for n, p in model.named_parameters()}
    oracle = w4a16_oracle(model)
    r = run_w4a16_engine(model, oracle, oracle, "cpu", 3, False)
    for n, p in model.named_parameters():       # a model passed in by the caller is left untouched
        assert torch.equal(p, before[n]), n
    assert r["d"] == 0.0 and r["bound"] == 3e-2        # both oracles are f32 here
    engine_checks(r, "cpu engine")
    assert max(r["rels"]) < 1e-4, max(r["rels"])       # f32 against f32: the same function
    assert r["same"]                                     # the greedy tokens are the oracle's
