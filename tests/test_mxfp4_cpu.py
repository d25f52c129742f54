"""MXFP4 weights x fp8 activations (--quantization mxfp4) on the CPU: the block quantizer on
hand-made blocks and on Gaussian data, the torch reference path of ``linear_nt``, flags, TP
slicing and the plan-table loader, and the engine end to end against the fake-quant oracle.  The
oracle and the engine harness below are shared with tests/test_mxfp4_gpu.py."""
import copy
import gc
import json

import pytest
import torch

from lumen.models import build_model
from lumen.serve.engine import EngineConfig, LLMEngine
from lumen.serve.model_runner import ServeWeights
from lumen.serve.sequence import SamplingParams
from tests.test_w8a8_cpu import PROMPTS, add_fake_quant_hooks, ptpc_model, rel

PROJ = ("self_attn.qkv_proj", "self_attn.o_proj", "mlp.gate_up_proj", "mlp.down_proj")
NAMES = ("qkv", "o", "gate_up", "down")
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def codes_of(qw):
    """[N, Kp] e2m1 codes of an Mxfp4Weight: the low nibble of a byte is the even k."""
    return torch.stack((qw.q & 0xF, qw.q >> 4), dim=-1).view(qw.q.shape[0], -1)


# ---- the oracle and the engine harness (shared with the GPU tests) ------------------------------

def mxfp4_oracle(m, f32=False):
    """A deep copy of ``m`` whose four projection weights are replaced by
    ``quantize_mxfp4_rows(w).dequant()`` and whose projection inputs go through
    ``quantize_fp8_tokens`` and back.  ``f32``: the same weights with f32 activations."""
    from lumen.ops.quant import quantize_mxfp4_rows

    d = copy.deepcopy(m)
    with torch.no_grad():
        for L in d.layers:
            for name in PROJ:
                lin = L.get_submodule(name)
                lin.weight.copy_(quantize_mxfp4_rows(lin.weight).dequant())
    return add_fake_quant_hooks(d.float() if f32 else d)


def run_mxfp4_engine(m, oracle, oracle32, device, nprompts, graphs, max_tokens=12, **kw):
    """tests/test_w8a8_cpu.run_ptpc_engine with quantization="mxfp4": serve ``nprompts`` prompts
    greedily and compare with the oracle's teacher-forced full forward.  Returns the same dict
    (rels, d, bound = max(3e-2, 2 d), own, agree, left_out)."""
    from lumen.ops.quant import Mxfp4Weight

    dev = torch.device(device)
    eng = LLMEngine(EngineConfig(model="tiny-llama-gqa", device=device, max_model_len=512,
                                 block_size=16, num_blocks=128, use_graphs=graphs,
                                 quantization="mxfp4", **kw), model=m)
    assert all(isinstance(getattr(L, n), Mxfp4Weight) for L in eng.weights.layers for n in NAMES)
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


def engine_checks(r, what):
    print(what, "d", r["d"], "bound", r["bound"], "max logits rel", max(r["rels"]), "rows",
          len(r["rels"]), "agreement", r["agree"], "left out", r["left_out"])
    assert len(r["rels"]) >= 10
    assert max(r["rels"]) < r["bound"], (max(r["rels"]), r["bound"])
    assert all(r["own"])
    assert r["left_out"] <= 0.25, r["left_out"]
    assert r["agree"] >= 0.9, r["agree"]


# ---- quantize_mxfp4_rows on hand-made blocks ------------------------------------------------------

def test_ties_round_to_the_even_code():
    from lumen.ops.quant import quantize_mxfp4_rows

    # the block maximum 4 gives e = 0: the values are their own scaled values
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    w = torch.zeros(2, 32)
    w[0, :7] = torch.tensor(ties)
    w[0, 31] = 4.0
    w[1, :7] = -torch.tensor(ties)
    w[1, 31] = -4.0
    qw = quantize_mxfp4_rows(w)
    assert qw.q.dtype == torch.uint8 and qw.q.shape == (2, 16)
    assert qw.scale.dtype == torch.uint8 and qw.scale.tolist() == [[127], [127]]
    d = qw.dequant()
    assert d[0, :7].tolist() == want and d[1, :7].tolist() == [-v for v in want]
    c = codes_of(qw)
    assert c[0, :7].tolist() == [0, 2, 2, 4, 4, 6, 6]          # every tie lands on an even code
    assert c[1, :7].tolist() == [0, 10, 10, 12, 12, 14, 14]    # sign = bit 3; no negative zero
    # every grid point is its own code
    w = torch.zeros(1, 32)
    w[0, :8] = torch.tensor(GRID)
    w[0, 8:16] = -torch.tensor(GRID)
    c = codes_of(quantize_mxfp4_rows(w))
    assert c[0, :16].tolist() == list(range(8)) + [0] + list(range(9, 16))


def test_block_exponent_clamp_and_zero_block():
    from lumen.ops.quant import quantize_mxfp4_rows

    js = list(range(-20, 21, 5))
    w = torch.zeros(len(js) * 2 + 2, 32)
    for i, j in enumerate(js):
        w[2 * i, 3] = 2.0 ** j                                    # amax = 2^j: e = j - 2
        w[2 * i + 1, 3] = -(2.0 ** j) * (1 - 2.0 ** -20)          # just below 2^j: e = j - 3
    w[-2, 0], w[-2, 1] = 7 * 2.0 ** 5, -3 * 2.0 ** 5              # 7 * 2^e clamps to 6 * 2^e
    qw = quantize_mxfp4_rows(w)
    e = qw.scale[:, 0].to(torch.int32) - 127
    for i, j in enumerate(js):
        assert e[2 * i] == j - 2 and e[2 * i + 1] == j - 3, (j, e[2 * i], e[2 * i + 1])
    d = qw.dequant()
    assert e[-2] == 5 and d[-2, 0] == 6 * 2.0 ** 5 and d[-2, 1] == -3 * 2.0 ** 5
    # an all-zero block: byte 127 and zero codes
    assert qw.scale[-1, 0] == 127 and int(qw.q[-1].sum()) == 0
    # the block exponent is clamped to E8M0's finite range
    tiny = quantize_mxfp4_rows(torch.full((1, 32), 2.0 ** -140))
    assert tiny.scale[0, 0] == 0
    with pytest.raises(ValueError):
        quantize_mxfp4_rows(torch.zeros(2, 3, 4))


def test_partial_block_nibble_order_and_round_trip():
    from lumen.ops.quant import Mxfp4Weight, quantize_mxfp4_rows

    w = torch.zeros(3, 48)
    w[0, 0], w[0, 1], w[0, 2], w[0, 3] = 1.0, -6.0, 3.0, 0.5     # block 0: e = 0
    w[0, 32], w[0, 47] = 8.0, -2.0                               # block 1 (16 valid k): e = 1
    qw = quantize_mxfp4_rows(w.to(torch.bfloat16))
    assert isinstance(qw, Mxfp4Weight) and qw.K == 48 and qw.dtype == torch.bfloat16
    assert tuple(qw.shape) == (3, 48) and qw.dim() == 2 and qw.device == w.device
    assert qw.q.shape == (3, 32) and qw.scale.shape == (3, 2)
    assert qw.nbytes == 3 * 32 + 3 * 2
    assert qw.scale[0].tolist() == [127, 128]
    # low nibble = even k: (1.0 -> 2, -6 -> 15), (3 -> 5, .5 -> 1)
    assert qw.q[0, 0] == 2 | (15 << 4) and qw.q[0, 1] == 5 | (1 << 4)
    assert qw.q[0, 16] == 6 and qw.q[0, 23] == (8 | 2) << 4      # 8 / 2 = 4 -> 6; -2 / 2 -> 8 | 2
    assert int(qw.q[0, 24:].sum()) == 0                          # padding nibbles are zero
    d = qw.dequant()
    assert d.shape == (3, 48) and d.dtype == torch.bfloat16 and torch.equal(d.float(), w)
    g = torch.Generator().manual_seed(1)
    for K in (48, 400):
        q1 = quantize_mxfp4_rows(torch.randn(16, K, generator=g) * torch.logspace(-3, 3, 16)[:, None])
        q2 = quantize_mxfp4_rows(q1.dequant())
        assert torch.equal(q1.q, q2.q) and torch.equal(q1.scale, q2.scale) and q2.K == K
        assert int(codes_of(q1)[:, K:].sum()) == 0


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
def test_quantizer_error_bound_on_gaussian(dt):
    """|w - wdq| <= amax_block / 2 for every element: the grid's step is at most 2 * 2^e, the
    clamp loses less than 2 * 2^e, and amax >= 4 * 2^e."""
    from lumen.ops.quant import quantize_mxfp4_rows

    g = torch.Generator().manual_seed(4)
    w = (torch.randn(64, 400, generator=g) * 0.02).to(dt)
    qw = quantize_mxfp4_rows(w)
    assert qw.q.shape == (64, 208) and qw.scale.shape == (64, 13)
    wf = torch.zeros(64, 416)
    wf[:, :400] = w.float()
    amax = wf.view(64, 13, 32).abs().amax(-1)
    wdq = qw.dequant_f32()
    err = (wf[:, :400] - wdq).abs().view(64, -1)
    bound = (amax / 2).repeat_interleave(32, dim=1)[:, :400]
    assert (err <= bound).all(), (err - bound).max().item()
    # the block maximum lands in [4, 8) * 2^e
    e = qw.scale.to(torch.int32) - 127
    scaled = torch.ldexp(amax, -e)
    assert ((scaled >= 4) & (scaled < 8)).all()
    print(dt, "relative weight error", rel(wdq, w))
    if dt == torch.bfloat16:
        assert torch.equal(qw.dequant().float(), wdq)


# ---- linear_nt ----------------------------------------------------------------------------------

def test_linear_nt_cpu_is_the_definition():
    from lumen.ops.activation import swiglu
    from lumen.ops.gemm import linear_nt, swiglu_linear_nt
    from lumen.ops.quant import (QuantWeight, quantize_fp8_rows, quantize_fp8_tokens,
                                 quantize_mxfp4_rows)

    g = torch.Generator().manual_seed(5)
    for dt, tol in ((torch.float32, 1e-6), (torch.bfloat16, 2.0 ** -8)):
        w = (torch.randn(68, 688, generator=g) * 0.02).to(dt)
        qw = quantize_mxfp4_rows(w)
        x = torch.randn(7, 688, generator=g).to(dt)
        xq, sx = quantize_fp8_tokens(x)
        wdq = torch.ldexp(torch.tensor(GRID + tuple(-v for v in GRID))[codes_of(qw).long()]
                          .view(68, -1, 32), (qw.scale.to(torch.int32) - 127)[:, :, None])
        ref = (xq.double() @ wdq.view(68, -1)[:, :688].double().t()) * sx.double()[:, None]
        y = linear_nt(x, qw)
        assert y.shape == (7, 68) and y.dtype == dt
        assert rel(y, ref) < tol
        # not the ptpc_fp8 function of the same inputs
        f8 = quantize_fp8_rows(w)
        assert rel(linear_nt(x, QuantWeight(f8.q, f8.scale, dt, act="fp8")), ref) > 1e-2
        gu = torch.randn(3, 2 * 688, generator=g).to(dt)
        assert torch.equal(swiglu_linear_nt(gu, qw), linear_nt(swiglu(gu), qw))


# ---- flags, config, TP, plan table ----------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    return ptpc_model(torch.float32, "cpu")


def test_serve_weights_and_config_accept_mxfp4(model):
    from lumen.ops.quant import Mxfp4Weight, quantize_mxfp4_rows

    plain = ServeWeights(model, 0, 1)
    w = ServeWeights(model, 0, 1, "mxfp4")
    assert w.quantization == "mxfp4"
    for Lp, Lq in zip(plain.layers, w.layers):
        for name in NAMES:
            qw, ref = getattr(Lq, name), quantize_mxfp4_rows(getattr(Lp, name))
            assert isinstance(qw, Mxfp4Weight) and tuple(qw.shape) == tuple(getattr(Lp, name).shape)
            assert torch.equal(qw.q, ref.q) and torch.equal(qw.scale, ref.scale)
    assert isinstance(w.lm_head, torch.Tensor) and torch.equal(w.lm_head, plain.lm_head)
    for bad in ("int3", "ptpc_fp4"):
        with pytest.raises(ValueError, match="mxfp4"):       # the message lists the new value
            ServeWeights(model, 0, 1, bad)
        with pytest.raises(ValueError, match="mxfp4"):
            LLMEngine(EngineConfig(model="tiny-llama-gqa", device="cpu", max_model_len=64,
                                   block_size=4, use_graphs=False, num_blocks=32,
                                   quantization=bad), model=model)
    assert EngineConfig(model="tiny-llama-gqa").quantization is None
    eng = LLMEngine(EngineConfig(model="tiny-llama-gqa", device="cpu", max_model_len=64,
                                 block_size=4, use_graphs=False, num_blocks=32,
                                 quantization="mxfp4"), model=model)
    assert eng.weights.quantization == "mxfp4"


def test_tp_rank_quantizes_its_own_slice():
    from lumen.ops.quant import quantize_mxfp4_rows

    m = build_model("tiny-llama-tp8", dtype=torch.bfloat16, device="cpu", init="random", seed=2)
    m.eval()
    for r in (0, 1):
        plain, quant = ServeWeights(m, r, 2), ServeWeights(m, r, 2, "mxfp4")
        for Lp, Lq in zip(plain.layers, quant.layers):
            for name in NAMES:
                qw, ref = getattr(Lq, name), quantize_mxfp4_rows(getattr(Lp, name))
                assert tuple(qw.shape) == tuple(ref.shape) == tuple(getattr(Lp, name).shape)
                assert torch.equal(qw.q, ref.q) and torch.equal(qw.scale, ref.scale), (r, name)


def test_cli_and_bench_accept_the_flag(monkeypatch):
    import sys

    from lumen.bench import serve_bench
    from lumen.cli.serve import build_parser

    p = build_parser()
    assert p.parse_args(["--model", "tiny-llama", "--quantization", "mxfp4"]
                        ).quantization == "mxfp4"
    assert p.parse_args(["--model", "tiny-llama"]).quantization is None
    for bad in ("int3", "ptpc_fp4", "ptpc"):
        with pytest.raises(SystemExit):
            p.parse_args(["--model", "tiny-llama", "--quantization", bad])
    # serve_bench parses in main(): stop it where it would build the engine
    seen = []

    class Stop(Exception):
        pass

    def make_engine(a):
        seen.append(a.quantization)
        raise Stop

    monkeypatch.setattr(serve_bench, "make_engine", make_engine)
    monkeypatch.setattr(sys, "argv", ["serve_bench", "--quantization", "mxfp4"])
    with pytest.raises(Stop):
        serve_bench.main()
    assert seen == ["mxfp4"]
    monkeypatch.setattr(sys, "argv", ["serve_bench", "--quantization", "int3"])
    with pytest.raises(SystemExit):
        serve_bench.main()


def test_plan_table_loader(tmp_path, monkeypatch):
    import lumen.ops.gemm as gm

    path = tmp_path / "plans.json"
    path.write_text(json.dumps({"plans": [
        {"N": 12288, "K": 4096, "BM": 16, "BN": 128, "S": 2},
        {"N": 4096, "K": 11008, "BM": 256, "BN": 64, "S": 3, "us": 55.0}]}))
    want = {(12288, 4096, 16): (128, 2), (4096, 11008, 256): (64, 3)}
    assert gm.load_w4a8_plans(str(path)) == want
    assert gm.load_w4a8_plans(str(tmp_path / "missing.json")) == {}
    monkeypatch.setenv("LUMEN_W4A8_PLANS", str(path))
    monkeypatch.setattr(gm, "_w4a8_plans", None)
    assert gm.w4a8_plans() == want
    # the shipped table lists compiled variants only
    monkeypatch.delenv("LUMEN_W4A8_PLANS")
    monkeypatch.setattr(gm, "_w4a8_plans", None)
    for (N, K, bm), (bn, s) in gm.w4a8_plans().items():
        assert bm in gm.W4A8_BNS and bn in gm.W4A8_BNS[bm] and 1 <= s <= -(-K // 128)
        assert K % 16 == 0 and N % 4 == 0
    assert set(gm.W4A8_BNS) == set(gm.W4A8_BMS) == {16, 64, 128, 256}
    # the BM = 16 default: two workgroups per CU at N = 4096, never more slices than k128 steps
    bn, s = gm.w4a8_default_plan(4096, 4096)
    assert bn in gm.W4A8_BNS[16] and -(-4096 // bn) * s >= 512
    for N, K in ((72, 400), (4096, 11008), (22016, 4096), (256, 16)):
        bn, s = gm.w4a8_default_plan(N, K)
        assert bn in gm.W4A8_BNS[16] and 1 <= s <= -(-K // 128)


# ---- engine -------------------------------------------------------------------------------------

def test_engine_cpu_mxfp4_matches_fake_quant_oracle(model):
    before = {n: p.clone() for n, p in model.named_parameters()}
    oracle = mxfp4_oracle(model)
    r = run_mxfp4_engine(model, oracle, oracle, "cpu", 3, False)
    for n, p in model.named_parameters():       # a model passed in by the caller is left untouched
        assert torch.equal(p, before[n]), n
    assert r["d"] == 0.0 and r["bound"] == 3e-2        # both oracles are f32 here
    engine_checks(r, "cpu engine")
