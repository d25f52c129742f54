"""MXFP4 KV cache (``kv_cache_dtype="mxfp4"``) on the CPU: the holder, the block sizing and the
engine end to end through the reference paths."""
import pytest
import torch

from lumen.models import build_model
from lumen.models.config import PRESETS, ModelConfig
from lumen.ops.attention import Mxfp4KV, rope_write_kv, write_kv_cache
from lumen.ops.quant import quantize_mxfp4_rows
from lumen.serve.engine import EngineConfig, LLMEngine
from lumen.serve.model_runner import kv_bytes_per_token
from lumen.serve.sequence import SamplingParams


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    m = build_model("tiny-llama-gqa", dtype=torch.float32, device="cpu", init="random", seed=1)
    # larger init so greedy outputs depend on context (random-init logits are near-uniform)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 2:
                p.mul_(5.0)
    m.eval()
    return m


def _engine(model, **kw):
    cfg = EngineConfig(model="tiny-llama-gqa", device="cpu", max_model_len=256, block_size=4,
                       use_graphs=False, kv_cache_dtype="mxfp4", **kw)
    return LLMEngine(cfg, model=model)


def test_holder_round_trip():
    """A written row reads back as quantize_mxfp4_rows(row).dequant_f32(); code and scale bytes are
    the quantizer's; a -1 slot is skipped; unwritten slots read as 0; the values are bf16 numbers
    and quantizing them again reproduces the bytes."""
    torch.manual_seed(0)
    nb, nkv, bs, D = 7, 3, 4, 64
    kc, vc = Mxfp4KV(nb, nkv, bs, D), Mxfp4KV(nb, nkv, bs, D)
    assert kc.shape == (nb, nkv, bs, D) and kc.codes.shape == (nb, nkv, bs, D // 2)
    assert kc.scale.shape == (nb, nkv, bs, D // 32)
    assert kc.nbytes == nb * nkv * bs * (D // 2 + D // 32)
    assert (kc.dequant_f32() == 0).all() and (kc.scale == 127).all()
    T = 9
    k = (torch.randn(T, nkv, D) * 3).bfloat16()
    v = torch.randn(T, nkv, D).bfloat16()
    k[2, 1] = 0                      # an all-zero row
    k[3, 0, 32:] = 0                 # a row with one all-zero block
    slots = torch.tensor([5, 0, 27, 13, -1, 9, 22, 2, 17])
    write_kv_cache(k, v, kc, vc, slots)
    ok = slots >= 0
    blk, off = slots[ok] // bs, slots[ok] % bs
    for src, cache in ((k, kc), (v, vc)):
        w = quantize_mxfp4_rows(src[ok].reshape(-1, D))
        assert torch.equal(cache.codes[blk, :, off].reshape(-1, D // 2), w.q)
        assert torch.equal(cache.scale[blk, :, off].reshape(-1, D // 32), w.scale)
        dq = cache.dequant_f32()
        assert torch.equal(dq[blk, :, off].reshape(-1, D), w.dequant_f32())
        assert torch.equal(dq, dq.bfloat16().float())
        again = quantize_mxfp4_rows(dq.reshape(-1, D))
        assert torch.equal(again.q, cache.codes.reshape(-1, D // 2))
        written = torch.zeros(nb, bs, dtype=torch.bool)
        written[blk, off] = True
        assert (dq[~written[:, None, :].expand(nb, nkv, bs)] == 0).all()
        assert torch.equal(cache.dequant_f32(torch.tensor([3, 1])), dq[[3, 1]])


def test_rope_write_matches_rope_then_write():
    """rope_write_kv over holders == over a 16-bit cache, then quantized: same qkv rows, and the
    cache holds the quantization of the written-back k and of v."""
    from lumen.ops.rope import rope_tables

    torch.manual_seed(1)
    nh, nkv, D, bs, nb, T = 4, 2, 64, 4, 6, 10
    qkv = torch.randn(T, (nh + 2 * nkv) * D).bfloat16()
    pos = torch.randint(0, 100, (T,), dtype=torch.int32)
    slots = torch.arange(T, dtype=torch.int64) + bs
    cos, sin = rope_tables(D, 512, 10000.0, torch.device("cpu"))
    kc, vc = Mxfp4KV(nb, nkv, bs, D), Mxfp4KV(nb, nkv, bs, D)
    kb = torch.zeros(nb, nkv, bs, D, dtype=torch.bfloat16)
    vb = torch.zeros_like(kb)
    x1, x2 = qkv.clone(), qkv.clone()
    rope_write_kv(x1, pos, nh, nkv, D, cos, sin, kc, vc, slots)
    rope_write_kv(x2, pos, nh, nkv, D, cos, sin, kb, vb, slots)
    assert torch.equal(x1, x2)
    for cache, ref in ((kc, kb), (vc, vb)):
        w = quantize_mxfp4_rows(ref.reshape(-1, D))
        assert torch.equal(cache.dequant_f32().reshape(-1, D), w.dequant_f32())


def test_block_sizing():
    """0.53125 bytes per element: D/2 + D/32 per head row; holders allocate exactly that."""
    cfg = ModelConfig(**PRESETS["tiny-llama-gqa"])
    D, nkv, L = cfg.head_dim, cfg.num_key_value_heads, cfg.num_hidden_layers
    assert kv_bytes_per_token(cfg, 17 / 32) == 2 * L * nkv * (D // 2 + D // 32)
    assert kv_bytes_per_token(cfg, 2) == 2 * L * nkv * D * 2
    assert kv_bytes_per_token(cfg, 1, 2) == 2 * L * (nkv // 2) * D
    llama7 = ModelConfig(**PRESETS["tiny-llama-gqa"])
    llama7.hidden_size, llama7.num_attention_heads, llama7.num_key_value_heads = 4096, 32, 32
    assert kv_bytes_per_token(llama7, 17 / 32) == 2 * L * 32 * 68
    bs, nb = 4, 11
    c = Mxfp4KV(nb, nkv, bs, D)
    assert 2 * L * c.nbytes == nb * bs * kv_bytes_per_token(cfg, 17 / 32)


def test_auto_blocks_use_the_byte_formula(model):
    """Unset num_blocks: the CPU budget (256 MiB) divided by the mxfp4 block bytes, capped by
    max_num_seqs x blocks per sequence + 64 -- 32/17 of the fp8 cache's count uncapped."""
    eng = _engine(model, max_num_seqs=4096)
    per_block = kv_bytes_per_token(model.config, 17 / 32) * 4
    assert eng.blocks.num_blocks == (256 << 20) // per_block
    r = eng.runner
    assert all(isinstance(c, Mxfp4KV) for c in r.k_cache + r.v_cache)
    assert sum(c.nbytes for c in r.k_cache + r.v_cache) == eng.blocks.num_blocks * per_block


def test_engine_generates(model):
    """End to end on the tiny model; the logits of a prefill + decode over the 4-bit cache stay in
    the neighbourhood of the 16-bit cache's (round to nearest, 11.7 % per element on Gaussian
    data)."""
    eng = _engine(model, num_blocks=200)
    assert isinstance(eng.runner.k_cache[0], Mxfp4KV)
    out = eng.generate([[5, 17, 33, 9], list(range(3, 60))],
                       SamplingParams(max_tokens=8, temperature=0.0))
    assert [len(o.output_ids) for o in out] == [8, 8]
    # the prompt's K/V really went into the cache
    assert any(int((c.codes != 0).sum()) > 0 for c in eng.runner.k_cache)



def _requantize(cache, slots):
    """Replace the rows of a plain cache at ``slots`` by their MXFP4 round trip."""
    s = slots.long()
    s = s[s >= 0]
    bs, D = cache.shape[2], cache.shape[3]
    blk, off = s // bs, s % bs
    rows = cache[blk, :, off]
    w = quantize_mxfp4_rows(rows.reshape(-1, D).float())
    cache[blk, :, off] = w.dequant_f32().view(rows.shape).to(cache.dtype)


def test_engine_matches_exact_oracle(model, monkeypatch):
    """Every dequantised value is representable in the plain cache's type and the quantizer is
    idempotent, so an engine whose plain cache holds the round trip of every written row is an
    exact oracle: on the CPU both run the same reference attention over the same values."""
    import lumen.serve.model_runner as mr

    def logits(kv):
        e = LLMEngine(EngineConfig(model="tiny-llama-gqa", device="cpu", max_model_len=256,
                                   block_size=4, use_graphs=False, num_blocks=200,
                                   kv_cache_dtype=kv), model=model)
        e.add_request(list(range(3, 40)), SamplingParams(max_tokens=4, temperature=0.0))
        e.step()
        return e.runner.execute(e._build_input(e.scheduler.schedule())).float()

    l4 = logits("mxfp4")
    plain = mr.rope_write_kv

    def oracle_write(qkv, positions, nh, nkv, D, cos, sin, kc, vc, slots):
        plain(qkv, positions, nh, nkv, D, cos, sin, kc, vc, slots)
        _requantize(kc, slots)
        _requantize(vc, slots)

    monkeypatch.setattr(mr, "rope_write_kv", oracle_write)
    lo = logits("auto")
    assert torch.isfinite(l4).all()
    assert ((l4 - lo).norm() / lo.norm()).item() < 1e-5


def test_prefix_caching_same_tokens(model):
    """Repeated-prefix prompts: greedy tokens with prefix caching on == off (cached blocks hold
    the same bytes a fresh write would)."""
    pre = list(range(10, 42))
    prompts = [pre + [100, 101], pre + [200, 201, 202], pre + [100, 101]]
    sp = SamplingParams(max_tokens=6, temperature=0.0)
    outs = []
    for on in (False, True):
        eng = _engine(model, num_blocks=200, enable_prefix_caching=on)
        toks = []
        for p in prompts:   # one after another, so later prompts find the prefix cached
            toks.append(eng.generate([p], sp)[0].output_ids)
        outs.append(toks)
    assert outs[0] == outs[1]


def test_speculative_and_chunked_same_tokens(model):
    """Prompt-lookup speculation (verify steps over the cache, rejected tokens rolled back by block
    id) and small prefill chunks give the plain greedy tokens."""
    prompts = [[5, 9, 33, 7] * 8, list(range(3, 50))]
    sp = SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True)
    outs = []
    for k in (0, 3):
        eng = _engine(model, num_blocks=200, num_speculative_tokens=k, max_num_batched_tokens=16)
        outs.append([o.output_ids for o in eng.generate(prompts, sp)])
        if k:
            assert eng.stats["spec_steps"] > 0
    assert outs[0] == outs[1]


def test_head_dim_not_divisible_by_32_refused():
    d = dict(PRESETS["tiny-llama-gqa"], hidden_size=192, name="d48")   # head_dim 48
    m = build_model(ModelConfig(**d), dtype=torch.float32, device="cpu", init="random", seed=1)
    m.eval()
    with pytest.raises(ValueError, match="head_dim % 32"):
        LLMEngine(EngineConfig(model="tiny-llama-gqa", device="cpu", max_model_len=64,
                               block_size=4, use_graphs=False, num_blocks=32,
                               kv_cache_dtype="mxfp4"), model=m)
    with pytest.raises(ValueError, match="head_dim"):
        Mxfp4KV(4, 2, 4, 48)
    # the other cache types still take it
    LLMEngine(EngineConfig(model="tiny-llama-gqa", device="cpu", max_model_len=64, block_size=4,
                           use_graphs=False, num_blocks=32, kv_cache_dtype="fp8"), model=m)
