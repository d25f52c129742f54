"""MXFP4 KV cache (``--kv-cache-dtype mxfp4``) on the GPU: the cache-write kernels store exactly
``quantize_mxfp4_rows`` of every head row, and the attention kernels over the 4-bit cache match
the f32 references over its dequantised values.  Every dequantised value is a bf16 number and the
quantizer is idempotent, so a 16-bit cache holding the dequantised values is an exact oracle."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (nh, nkv, D, block size): the fp8 cache test's shapes at its block size; block size 32, which at
# D = 128 is not the decode kernel's rows per step (the per-lane block-table form) and at D = 64
# is (the uniform-block-id form); D = 32 (one MX block a row: the fused write's lane-pair form)
# and D = 256 (32 lanes a row)
SHAPES = [(32, 32, 128, 16), (64, 8, 128, 16), (12, 12, 64, 16), (32, 32, 128, 32),
          (64, 8, 128, 32), (12, 12, 64, 32), (8, 4, 32, 16), (4, 2, 256, 16)]
LENS = [300, 17, 200, 129]


@pytest.fixture(autouse=True)
def _native():
    from lumen.ops._native import native, native_error

    assert native() is not None, f"native extension must load on the GPU box: {native_error()!r}"
    torch.manual_seed(0)


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _special_rows(T, nkv, D, dtype):
    """[T, nkv, D] Gaussian rows (K-like, x3) with the quantizer's edge cases planted in the
    first tokens of every head: block 0 of the row carries the pattern."""
    x = (torch.randn(T, nkv, D, device=DEV) * 3).to(dtype)
    grid = torch.tensor([5, 2.5, 1.25, 0.25, 0.75, 1.75, 3.5, 4, -5, -2.5, -1.25, -0.25, -0.75,
                         -1.75, -3.5, -4, 0, 3, -3, 0.5, 1, 1.5, 2, 6, -6, 4.5, -4.5, 2.25, -2.25,
                         0.125, -0.125, 5.5], device=DEV)          # code midpoints and grid points
    over = torch.tensor([7, 6.5, 7.5, -7, 6.25, -7.75, 6, -6] * 4, device=DEV)   # (6, 8) 2^e
    pow2 = torch.tensor([1.0, 0.25, -0.5, 0.875, -1.0, 0.3125, 0.4375, 0.1875] * 4, device=DEV)
    x[0] = 0                                       # an all-zero row
    x[1, :, :32] = 0                               # a row with one all-zero block
    x[2, :, :32] = -x[2, :, :32].abs() - 0.01      # a negative-only block
    x[3, :, :32] = (grid * 2.0 ** -3).to(dtype)    # ties, at three block exponents
    x[4, :, :32] = grid.to(dtype)
    x[5, :, :32] = (grid * 2.0 ** 5).to(dtype)
    x[6, :, :32] = (over * 2.0 ** -2).to(dtype)    # clamped at 6
    x[7, :, :32] = (over * 2.0 ** 3).to(dtype)
    x[8, :, :32] = (pow2 * 2.0 ** 4).to(dtype)     # amax an exact power of two
    x[9, :, :32] = (pow2 * 2.0 ** -6).to(dtype)
    x[10, :, -32:] = (grid.flip(0) * 2.0).to(dtype)   # and in the row's last block
    return x


def _scatter_slots(T, bs, nblocks, skip=()):
    """T distinct slots over scattered blocks; ``skip`` tokens get -1."""
    g = torch.Generator().manual_seed(3)
    slots = torch.randperm(nblocks * bs, generator=g)[:T].to(DEV)
    for t in skip:
        slots[t] = -1
    return slots


def _noise_cache(nblocks, nkv, bs, D):
    """A holder whose bytes are random: whatever a kernel leaves alone stays recognisable."""
    from lumen.ops.attention import Mxfp4KV

    c = Mxfp4KV(nblocks, nkv, bs, D, DEV)
    c.buf.copy_(torch.randint(0, 256, c.buf.shape, device=DEV, dtype=torch.uint8))
    return c


def _expected(cache, rows, slots):
    """A copy of ``cache`` with quantize_mxfp4_rows(rows) stored at the valid slots (torch)."""
    from lumen.ops.attention import Mxfp4KV

    nb, nkv, bs, D = cache.shape
    e = Mxfp4KV(nb, nkv, bs, D, DEV)
    e.buf.copy_(cache.buf)
    ok = slots >= 0
    e.write(rows[ok], slots[ok] // bs, slots[ok] % bs)
    return e


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nh,nkv,D,bs", SHAPES)
def test_cache_write_bit_exact(nh, nkv, D, bs, dtype):
    """write_kv_cache: code bytes and scale bytes equal quantize_mxfp4_rows of every (token, head)
    row, every other byte of the cache (the -1 slots' would-be targets included) is untouched."""
    from lumen.ops.attention import write_kv_cache

    T, nblocks = 45, 9
    k = _special_rows(T, nkv, D, dtype)
    v = _special_rows(T, nkv, D, dtype).flip(0).contiguous()
    slots = _scatter_slots(T, bs, nblocks, skip=(4, 20))
    kc, vc = _noise_cache(nblocks, nkv, bs, D), _noise_cache(nblocks, nkv, bs, D)
    ek, ev = _expected(kc, k, slots), _expected(vc, v, slots)
    # strided rows, as the engine's views into the fused qkv buffer are
    kv = torch.cat([k, v], 1).contiguous()
    write_kv_cache(kv[:, :nkv], kv[:, nkv:], kc, vc, slots)
    assert torch.equal(kc.codes, ek.codes) and torch.equal(kc.scale, ek.scale)
    assert torch.equal(vc.codes, ev.codes) and torch.equal(vc.scale, ev.scale)
    assert torch.equal(kc.buf, ek.buf) and torch.equal(vc.buf, ev.buf)
    # and the holder reads back what the definition dequantises to
    ok = slots >= 0
    from lumen.ops.quant import quantize_mxfp4_rows

    got = kc.dequant_f32()[slots[ok] // bs, :, slots[ok] % bs]
    assert torch.equal(got.reshape(-1, D), quantize_mxfp4_rows(k[ok].reshape(-1, D)).dequant_f32())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nh,nkv,D,bs", SHAPES)
def test_fused_rope_write_bit_exact(nh, nkv, D, bs, dtype):
    """rope_write_kv over holders: the qkv rows equal the 16-bit-cache call's, K holds the
    quantization of the written-back (rounded) k rows, V the quantization of the v rows."""
    from lumen.ops.attention import rope_write_kv
    from lumen.ops.rope import rope_tables

    T, nblocks = 50, 9
    qkv = torch.randn(T, (nh + 2 * nkv) * D, device=DEV).to(dtype)
    qkv[:, (nh + nkv) * D:] = _special_rows(T, nkv, D, dtype).view(T, nkv * D)
    pos = torch.randint(0, 400, (T,), device=DEV, dtype=torch.int32)
    slots = _scatter_slots(T, bs, nblocks, skip=(7,))
    cos, sin = rope_tables(D, 4096, 10000.0, DEV)
    kc, vc = _noise_cache(nblocks, nkv, bs, D), _noise_cache(nblocks, nkv, bs, D)
    kb = torch.zeros(nblocks, nkv, bs, D, device=DEV, dtype=dtype)
    vb = torch.zeros_like(kb)
    k0, v0 = kc.buf.clone(), vc.buf.clone()
    x1, x2 = qkv.clone(), qkv.clone()
    rope_write_kv(x1, pos, nh, nkv, D, cos, sin, kc, vc, slots)
    rope_write_kv(x2, pos, nh, nkv, D, cos, sin, kb, vb, slots)
    assert torch.equal(x1, x2)
    kr = x2[:, nh * D:(nh + nkv) * D].reshape(T, nkv, D)
    vr = x2[:, (nh + nkv) * D:].reshape(T, nkv, D)
    kc0, vc0 = _noise_cache(nblocks, nkv, bs, D), _noise_cache(nblocks, nkv, bs, D)
    kc0.buf.copy_(k0)
    vc0.buf.copy_(v0)
    ek, ev = _expected(kc0, kr, slots), _expected(vc0, vr, slots)
    assert torch.equal(kc.codes, ek.codes) and torch.equal(kc.scale, ek.scale)
    assert torch.equal(vc.codes, ev.codes) and torch.equal(vc.scale, ev.scale)
    assert torch.equal(kc.buf, ek.buf) and torch.equal(vc.buf, ev.buf)


@functools.lru_cache(maxsize=None)
def _filled(nh, nkv, D, bs):
    """Holders filled through the torch definition (so the attention tests do not lean on the
    write kernels), the scattered block table, and the dequantised caches -- built once."""
    from lumen.ops.attention import Mxfp4KV

    g = torch.Generator(device=DEV).manual_seed(11)
    nseq, ctx = len(LENS), max(LENS)
    maxb = (ctx + bs - 1) // bs
    nblocks = nseq * maxb + 5
    kc, vc = Mxfp4KV(nblocks, nkv, bs, D, DEV), Mxfp4KV(nblocks, nkv, bs, D, DEV)
    perm = torch.randperm(nblocks, generator=torch.Generator().manual_seed(5))[: nseq * maxb]
    perm = perm.view(nseq, maxb).int().to(DEV)
    for i, L in enumerate(LENS):
        k = (torch.randn(L, nkv, D, device=DEV, generator=g) * 3).bfloat16()
        v = torch.randn(L, nkv, D, device=DEV, generator=g).bfloat16()
        t = torch.arange(L, device=DEV)
        kc.write(k, perm[i, t // bs].long(), t % bs)
        vc.write(v, perm[i, t // bs].long(), t % bs)
    return kc, vc, perm, kc.dequant_f32(), vc.dequant_f32()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nh,nkv,D,bs", SHAPES)
def test_paged_decode(nh, nkv, D, bs, dtype):
    """paged_decode over the holders vs the f32 reference over dequant_f32(): identical cache
    values, so the only error is the sum order and the output rounding (the bound of the fp8
    cache's test for the same comparison)."""
    from lumen.ops.attention import paged_decode, paged_decode_ref

    kc, vc, perm, kd, vd = _filled(nh, nkv, D, bs)
    q = torch.randn(len(LENS), nh, D, device=DEV).to(dtype)
    cl = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    scale = 1 / math.sqrt(D)
    ref = paged_decode_ref(q.float(), kd, vd, perm, cl, scale)
    # the reference functions take the holder too (they dequantise the gathered blocks)
    assert torch.equal(paged_decode_ref(q.float(), kc, vc, perm, cl, scale), ref)
    for part in (512, 64):
        for one in (0, 1, 2, 3):
            got = paged_decode(q, kc, vc, perm, cl, max(LENS), scale, part, one_pass=one)
            r = rel(got, ref)
            print(f"decode nh={nh} nkv={nkv} D={D} bs={bs} part={part} one_pass={one} rel={r:.2e}")
            assert r < 1e-2, (one, part, r)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nh,nkv,D,bs", [s for s in SHAPES if s[2] == 128])
def test_chunked_prefill(nh, nkv, D, bs, dtype):
    """flash_attention_paged over the holders (blocks dequantised into the 16-bit scratch: exact in
    bf16, one rounding in fp16) vs its reference over the dequantised cache."""
    from lumen.ops.attention import flash_attention_paged, flash_attention_paged_ref

    kc, vc, perm, kd, vd = _filled(nh, nkv, D, bs)
    cu, kl = [0, 20, 37, 137, 138], LENS
    qr = (torch.randn(cu[-1], (nh + 2 * nkv) * D, device=DEV) * 0.5).to(dtype)
    got = flash_attention_paged(qr, kc, vc, cu, kl, perm, nh, nkv, D)
    ref = flash_attention_paged_ref(qr.float(), kd, vd, cu, kl, perm, nh, nkv, D)
    r = rel(got, ref)
    print(f"prefill nh={nh} nkv={nkv} bs={bs} rel={r:.2e}")
    assert r < 1e-2, r
    assert torch.equal(flash_attention_paged_ref(qr.float(), kc, vc, cu, kl, perm, nh, nkv, D), ref)


def test_dequant_scratch_exact():
    """The prefill scratch holds exactly the dequantised blocks (bf16)."""
    from lumen.ops.attention import _dequant_blocks

    nh, nkv, D, bs = 64, 8, 128, 16
    kc, vc, perm, kd, vd = _filled(nh, nkv, D, bs)
    kl = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    ks, vs, ident = _dequant_blocks(kc, vc, perm, kl, torch.bfloat16)
    for s, L in enumerate(LENS):
        n = (L + bs - 1) // bs
        assert torch.equal(ks[ident[s, :n].long()].float(), kd[perm[s, :n].long()])
        assert torch.equal(vs[ident[s, :n].long()].float(), vd[perm[s, :n].long()])


def _tiny_model():
    from lumen.models import build_model

    m = build_model("tiny-llama-gqa", dtype=torch.bfloat16, device=torch.device("cuda", 0),
                    init="random", seed=3)
    m.eval()
    return m


def _requantize(cache, slots):
    """Replace the rows of a 16-bit cache at ``slots`` by their MXFP4 round trip (exact in bf16)."""
    from lumen.ops.quant import quantize_mxfp4_rows

    s = slots.long()
    s = s[s >= 0]
    bs, D = cache.shape[2], cache.shape[3]
    blk, off = s // bs, s % bs
    rows = cache[blk, :, off]
    w = quantize_mxfp4_rows(rows.reshape(-1, D))
    cache[blk, :, off] = w.dequant_f32().view(rows.shape).to(cache.dtype)


def test_engine_matches_exact_oracle(monkeypatch):
    """The mxfp4 engine against the same engine over a 16-bit cache that holds the MXFP4 round
    trip of every row its two cache-write entry points store: identical cache values, two kernels
    (the bound of test_fresh_prompt_prefill_matches_paged for that situation).  Both engines are
    fed the same token stream, so their decode steps see the same inputs."""
    import lumen.ops.attention as att
    import lumen.serve.model_runner as mr
    from lumen.serve.engine import EngineConfig, LLMEngine
    from lumen.serve.sequence import SamplingParams

    m = _tiny_model()
    prompts = [list(range(3, 200)), [5, 9, 33, 7] * 20, list(range(100, 140))]

    def decode_logits(kv):
        eng = LLMEngine(EngineConfig(model="tiny-llama-gqa", device="cuda", max_model_len=512,
                                     block_size=16, num_blocks=128, use_graphs=False,
                                     max_num_batched_tokens=1024, kv_cache_dtype=kv), model=m)
        got, n = [], [0]
        decode, sample = eng.runner.decode, eng.runner.sample

        def spy(inp):
            out = decode(inp)
            got.append(out.float().clone())
            return out

        def fixed(logits, *a, **k):
            t, lp = sample(logits, *a, **k)
            n[0] += 1
            t.copy_((torch.arange(t.shape[0], device=t.device) * 37 + n[0] * 11) % 400 + 3)
            return t, lp

        eng.runner.decode, eng.runner.sample = spy, fixed
        for p in prompts:
            eng.add_request(p, SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True))
        while eng.has_work:
            eng.step()
        return got

    a = decode_logits("mxfp4")
    rope_w, plain_w = mr.rope_write_kv, att.write_kv_cache

    def oracle_rope(qkv, positions, nh, nkv, D, cos, sin, kc, vc, slots):
        rope_w(qkv, positions, nh, nkv, D, cos, sin, kc, vc, slots)
        _requantize(kc, slots)
        _requantize(vc, slots)

    def oracle_write(k, v, kc, vc, slots):
        plain_w(k, v, kc, vc, slots)
        _requantize(kc, slots)
        _requantize(vc, slots)

    monkeypatch.setattr(mr, "rope_write_kv", oracle_rope)
    monkeypatch.setattr(att, "write_kv_cache", oracle_write)
    b = decode_logits("auto")
    assert len(a) == len(b) >= 4
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape == (3, m.config.vocab_size)
        r = rel(x, y)
        print(f"decode step {i}: rel {r:.2e}")
        assert r < 2e-2, (i, r)


def test_graphs_same_tokens():
    """hipGraph decode over the mxfp4 cache (static cache pointers) == eager decode."""
    from lumen.serve.engine import EngineConfig, LLMEngine
    from lumen.serve.sequence import SamplingParams

    m = _tiny_model()
    g = torch.Generator().manual_seed(9)
    prompts = [torch.randint(3, 500, (int(n),), generator=g).tolist()
               for n in torch.randint(10, 40, (8,), generator=g)]
    outs = []
    for graphs in (False, True):
        eng = LLMEngine(EngineConfig(model="tiny-llama-gqa", device="cuda", max_model_len=256,
                                     block_size=16, num_blocks=128, use_graphs=graphs,
                                     max_num_seqs=8, kv_cache_dtype="mxfp4"), model=m)
        assert eng.runner.use_graphs == graphs
        res = eng.generate(prompts, SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True))
        outs.append([r.output_ids for r in res])
    assert outs[0] == outs[1]
