"""fp8 weight-only quantization (--quantization fp8) on the CPU: the quantizer's error bounds,
the torch reference path of ``linear_nt``, the engine end to end, TP slicing and the plan-table
loader."""
import copy
import json

import pytest
import torch

from lumen.models import build_model
from lumen.ops.gemm import linear_nt, load_w8_plans
from lumen.ops.quant import QuantWeight, quantize_fp8_rows
from lumen.serve.engine import EngineConfig, LLMEngine
from lumen.serve.model_runner import ServeWeights
from lumen.serve.sequence import SamplingParams

PROJ = ("self_attn.qkv_proj", "self_attn.o_proj", "mlp.gate_up_proj", "mlp.down_proj")


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


@pytest.mark.parametrize("N,K", [(68, 688), (1032, 256), (4096, 4096)])
def test_quantizer_bounds(N, K):
    g = torch.Generator().manual_seed(N + K)
    w = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16)
    qw = quantize_fp8_rows(w)
    assert qw.q.dtype == torch.float8_e4m3fn and qw.q.shape == (N, K) and qw.q.is_contiguous()
    assert qw.scale.dtype == torch.float32 and qw.scale.shape == (N,)
    assert qw.dtype == torch.bfloat16 and tuple(qw.shape) == (N, K)
    assert qw.nbytes == N * K + 4 * N
    qf = qw.q.float()
    assert not torch.isnan(qf).any() and torch.isfinite(qw.scale).all()
    # the row maximum maps to +-448
    assert torch.equal(qf.abs().amax(1), torch.full((N,), 448.0))
    # e4m3 has 3 mantissa bits: half an ulp is at most 1/17 of the value (< 2^-4); the second
    # term is half the subnormal spacing (2^-9 in units of the scale).  Checked on the f32
    # product, before dequant()'s rounding to bf16.
    wf = w.float()
    dq = qf * qw.scale[:, None]
    bound = wf.abs() * 2.0 ** -4 + qw.scale[:, None] * 2.0 ** -10
    assert ((dq - wf).abs() <= bound).all(), ((dq - wf).abs() - bound).max().item()
    assert qw.dequant().dtype == torch.bfloat16
    assert torch.equal(qw.dequant(), dq.to(torch.bfloat16))
    # and on the 16-bit weight the kernels' fallback multiplies by
    err16 = (qw.dequant().float() - wf).abs()
    assert (err16 <= bound).all(), (err16 - bound).max().item()


def test_quantizer_zero_row_and_outlier():
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(8, 64, generator=g) * 0.02).to(torch.bfloat16)
    w[2] = 0
    w[5, 7] = 1e4
    w[6, 9] = -1e4
    qw = quantize_fp8_rows(w)
    qf = qw.q.float()
    assert not torch.isnan(qf).any()
    assert torch.isfinite(qw.scale).all() and (qw.scale > 0).all()
    assert (qf[2] == 0).all() and (qw.dequant()[2] == 0).all()
    assert qf[5, 7] == 448.0 and qf[6, 9] == -448.0
    assert not torch.isnan(qw.dequant().float()).any()


def test_linear_nt_cpu_matches_dequant():
    g = torch.Generator().manual_seed(5)
    for dt in (torch.float32, torch.bfloat16):
        w = (torch.randn(68, 688, generator=g) * 0.02).to(dt)
        qw = quantize_fp8_rows(w)
        x = torch.randn(7, 688, generator=g)
        y = linear_nt(x, qw)
        assert y.shape == (7, 68) and y.dtype == x.dtype
        assert rel(y, x.float() @ qw.dequant().float().t()) < 1e-6


@pytest.fixture(scope="module")
def model():
    m = build_model("tiny-llama-gqa", dtype=torch.float32, device="cpu", init="random", seed=1)
    # larger init so greedy outputs depend on context (random-init logits are near-uniform)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 2:
                p.mul_(5.0)
    return m.eval()


def dequantized_copy(m):
    """A copy of ``m`` whose projection weights are replaced by their fp8 round trip."""
    d = copy.deepcopy(m)
    with torch.no_grad():
        for L in d.layers:
            for name in PROJ:
                lin = L.get_submodule(name)
                lin.weight.copy_(quantize_fp8_rows(lin.weight).dequant())
    return d


def _run(model, prompts, **kw):
    eng = LLMEngine(EngineConfig(model="tiny-llama-gqa", device="cpu", max_model_len=256,
                                 block_size=4, use_graphs=False, num_blocks=256, **kw),
                    model=model)
    logits = []
    for name in ("decode", "execute"):
        orig = getattr(eng.runner, name)

        def spy(inp, orig=orig):
            out = orig(inp)
            logits.append(out.float().clone())
            return out
        setattr(eng.runner, name, spy)
    seqs = eng.generate(prompts, SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True))
    return eng, [s.output_ids for s in seqs], logits[-1]


def test_engine_cpu_fp8_matches_dequantized_model(model):
    before = {n: p.clone() for n, p in model.named_parameters()}
    prompts = [[5, 9, 33, 7], list(range(3, 40)), [42]]
    eng, out_q, lg_q = _run(model, prompts, quantization="fp8")
    for L in eng.weights.layers:
        for w in (L.qkv, L.o, L.gate_up, L.down):
            assert isinstance(w, QuantWeight) and w.q.dtype == torch.float8_e4m3fn
    assert not isinstance(eng.weights.lm_head, QuantWeight)
    # a model passed in by the caller is left untouched
    for n, p in model.named_parameters():
        assert torch.equal(p, before[n]), n
    _, out_d, lg_d = _run(dequantized_copy(model), prompts)
    assert out_q == out_d
    assert lg_q.shape == lg_d.shape
    # both sides f32: they differ only by where the scale multiplies
    assert rel(lg_q, lg_d) < 1e-4


def test_engine_default_is_unquantized(model):
    assert EngineConfig().quantization is None
    eng = LLMEngine(EngineConfig(model="tiny-llama-gqa", device="cpu", max_model_len=64,
                                 block_size=4, use_graphs=False, num_blocks=32), model=model)
    assert eng.weights.quantization is None
    assert all(isinstance(L.qkv, torch.Tensor) for L in eng.weights.layers)


def test_unknown_quantization_raises(model):
    with pytest.raises(ValueError):
        LLMEngine(EngineConfig(model="tiny-llama-gqa", device="cpu", max_model_len=64,
                               block_size=4, use_graphs=False, num_blocks=32,
                               quantization="int3"), model=model)
    with pytest.raises(ValueError):
        ServeWeights(model, 0, 1, "int3")


def test_cli_accepts_quantization_flag():
    from lumen.cli.serve import build_parser

    assert build_parser().parse_args(["--model", "tiny-llama", "--quantization", "fp8"]
                                     ).quantization == "fp8"
    assert build_parser().parse_args(["--model", "tiny-llama"]).quantization is None
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--model", "tiny-llama", "--quantization", "int3"])


def test_tp_slices_are_quantized_after_slicing():
    m = build_model("tiny-llama-tp8", dtype=torch.bfloat16, device="cpu", init="random", seed=2)
    m.eval()
    for r in (0, 1):
        plain = ServeWeights(m, r, 2)
        quant = ServeWeights(m, r, 2, "fp8")
        for Lp, Lq in zip(plain.layers, quant.layers):
            for name in ("qkv", "o", "gate_up", "down"):
                w16, qw = getattr(Lp, name), getattr(Lq, name)
                ref = quantize_fp8_rows(w16)   # this rank's slice, its own row maxima
                N, K = w16.shape
                assert tuple(qw.shape) == (N, K) and qw.dtype == torch.bfloat16
                assert torch.equal(qw.q.view(torch.uint8), ref.q.view(torch.uint8)), (r, name)
                assert torch.equal(qw.scale, ref.scale), (r, name)
                assert qw.nbytes == N * K + 4 * N
        assert quant.lm_head.dtype == torch.bfloat16 and quant.embed.dtype == torch.bfloat16


def test_plan_table_loader(tmp_path):
    path = tmp_path / "plans.json"
    path.write_text(json.dumps({"plans": [
        {"N": 12288, "K": 4096, "BM": 64, "BN": 64, "S": 2},
        {"N": 4096, "K": 11008, "BM": 256, "BN": 64, "S": 3, "us": 55.0}]}))
    assert load_w8_plans(str(path)) == {(12288, 4096, 64): (64, 2), (4096, 11008, 256): (64, 3)}
    assert load_w8_plans(str(tmp_path / "missing.json")) == {}
