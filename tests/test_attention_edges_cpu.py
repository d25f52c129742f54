"""The builders and references of the attention edge tests (``_attn_cases.py``,
``test_attention_edges_gpu.py``) on the CPU, over the exact case lists the GPU tests use: the
references are finite wherever the GPU tests check them, every cache really holds poison, and the
per-sequence metric and the NaN-filling ``torch.empty`` behave as documented."""
import math

import pytest
import torch

from _attn_cases import (BS, CHUNK_LENS, CTX_LENS, D, HEADS, KINDS, VARLEN_LENS, WIDE_BOOST,
                         PagedCase, block_table, cache_f32, cu_of, dominant_key, nan_empty,
                         nan_rows, poison_share, poisoned_cache, seq_err, varlen_qkv, wide_q)
from lumen.ops.attention import (FP8_KV, Mxfp4KV, flash_attention_paged_ref, flash_attention_ref,
                                 paged_decode_ref)

DTYPES = [torch.bfloat16, torch.float16]


def _ref_fwd_bwd(qkv, do, cu, nh, nkv, causal):
    x = qkv.float().requires_grad_(True)
    o = flash_attention_ref(x, tuple(cu), nh, nkv, D, causal)
    (g,) = torch.autograd.grad(o, x, do.float())
    return o.detach(), g


def test_seq_err_metric():
    cu = cu_of([1, 3, 60])
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(64, 32, generator=g)
    ref[0] = 0                                  # an exactly-zero reference sequence
    ref[1:4] *= 2                               # sequence 1 stands above the floor: own norm
    assert seq_err(ref, ref, cu) == [0.0, 0.0, 0.0]
    got = ref.clone()
    got[0] = torch.randn(32, generator=g)       # garbage of a typical row's size there: about 1
    e = seq_err(got, ref, cu)
    assert 0.5 < e[0] < 2.0 and e[1] == 0.0 and e[2] == 0.0
    got = ref.clone()
    got[0] += 1e-6                              # rounding noise: about 0
    assert seq_err(got, ref, cu)[0] < 1e-5
    got = ref.clone()
    got[9, 5] = float("nan")                   # a NaN never passes a `<` bound
    e = seq_err(got, ref, cu)
    assert not e[2] < 1e9 and e[0] == 0.0 and e[1] == 0.0
    # a small sequence's error is not diluted by a large neighbour: 10 % on sequence 1
    got = ref.clone()
    got[1:4] *= 1.1
    e1 = seq_err(got, ref, cu)[1]
    assert abs(e1 - 0.1) < 1e-6
    assert ((got - ref).norm() / ref.norm()).item() < 0.6 * e1   # the global metric dilutes it


def test_nan_empty_poisons_and_restores():
    empty, empty_like = torch.empty, torch.empty_like
    with nan_empty():
        assert torch.empty(3, 5).isnan().all()
        assert torch.empty(3, 5, dtype=torch.bfloat16).isnan().all()
        assert torch.empty_like(torch.zeros(4)).isnan().all()
        assert (torch.empty(7, dtype=torch.uint8) == 0x7F).all()
        assert (torch.empty(7, dtype=FP8_KV).view(torch.uint8) == 0x7F).all()
        assert torch.empty(7, dtype=FP8_KV).float().isnan().all()
        assert torch.empty(2, dtype=torch.int32).dtype == torch.int32   # integers: left alone
        assert torch.empty(0).numel() == 0
    assert torch.empty is empty and torch.empty_like is empty_like
    with pytest.raises(RuntimeError):
        with nan_empty():
            raise RuntimeError("x")
    assert torch.empty is empty and torch.empty_like is empty_like


@pytest.mark.parametrize("kind", KINDS)
def test_poisoned_cache_is_all_poison(kind):
    c = poisoned_cache(kind, 5, 2, BS, D, torch.bfloat16)
    assert not torch.isfinite(cache_f32(c)).any()
    if kind == "fp8":
        assert c.dtype == FP8_KV and (c.view(torch.uint8) == 0x7F).all()
    if kind == "mxfp4":
        assert isinstance(c, Mxfp4KV)
        assert (c.codes == 0x77).all() and (c.scale == 0xFF).all()


def test_block_tables_are_valid():
    for lens, bs in ((CTX_LENS, BS), (CTX_LENS, 32)):
        bt, nblocks = block_table(lens, bs, 7)
        nblk = [(L + bs - 1) // bs for L in lens]
        live = torch.cat([bt[i, :n] for i, n in enumerate(nblk)])
        assert sorted(live.tolist()) == list(range(1, sum(nblk) + 1))   # a permutation of 1..
        assert live.tolist() != sorted(live.tolist())                  # shuffled
        for i, n in enumerate(nblk):
            assert (bt[i, n:] == 0).all()                               # padded with block 0
        assert 0 <= int(bt.min()) and int(bt.max()) < nblocks            # every id a valid index


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("kind", KINDS)
def test_paged_references_over_poison(kind, nh, nkv, dtype):
    """paged_decode_ref / flash_attention_paged_ref over the poisoned caches, plain and wide."""
    scale = 1 / math.sqrt(D)
    cu = cu_of(CHUNK_LENS)
    g = torch.Generator().manual_seed(1)
    for wide in (False, True):
        case = PagedCase(kind, CTX_LENS, nkv, BS, D, dtype, seed=3, wide=wide)
        share = poison_share(case.kc)
        print(f"{kind} wide={wide}: poisoned share of the dequantised cache {share:.3%}")
        assert 0.01 < share < 0.2 and poison_share(case.vc) > 0.01
        kd = cache_f32(case.kc)
        assert not torch.isfinite(kd[0]).any()                           # block 0: all poison
        for i, L in enumerate(CTX_LENS):                                # live slots: finite
            t = torch.arange(L)
            assert torch.isfinite(kd[case.bt[i, t // BS].long(), :, t % BS]).all()
            if L % BS:                                                   # the last block's tail
                assert not torch.isfinite(kd[case.bt[i, (L - 1) // BS].long(), :, L % BS:]).any()
        q = torch.randn(len(CTX_LENS), nh, D, generator=g).to(dtype)
        if wide:
            q = wide_q(q).to(dtype)
        ref = paged_decode_ref(q.float(), case.kc, case.vc, case.bt, case.cl, scale)
        assert torch.isfinite(ref).all()
        assert seq_err(ref, ref, range(len(CTX_LENS) + 1)) == [0.0] * len(CTX_LENS)
        if wide:
            # head 0 of the longest sequence: the last key's score stands tens above the rest
            keys = kd[case.bt[-1].long(), 0].reshape(-1, D)[:CTX_LENS[-1]]
            s = keys @ q[-1, 0].float() * scale
            assert q[-1, 0, 0].item() * keys[-1, 0].item() * scale > 30   # (mxfp4 rounds 28 to 24)
            assert (keys[:-1, 0] == 0).all() and (s.max() - s.min()).item() > 60
            continue
        qr = (torch.randn(cu[-1], (nh + 2 * nkv) * D, generator=g) * 0.5).to(dtype)
        qr[:, nh * D:] = float("nan")     # the chunk's k | v columns: the cache holds them
        ref = flash_attention_paged_ref(qr.float(), case.kc, case.vc, cu, CTX_LENS, case.bt, nh,
                                        nkv, D)
        assert ref.shape == (cu[-1], nh * D) and torch.isfinite(ref).all()
        assert seq_err(ref, ref, cu) == [0.0] * len(CHUNK_LENS)


def test_paged_case_d64_block32():
    """The extra decode shape (D = 64, block size 32: the uniform variants' block size there)."""
    case = PagedCase("16bit", CTX_LENS, 2, 32, 64, torch.bfloat16, seed=5)
    assert poison_share(case.kc) > 0.01
    q = torch.randn(len(CTX_LENS), 8, 64).bfloat16()
    ref = paged_decode_ref(q.float(), case.kc, case.vc, case.bt, case.cl, 0.125)
    assert torch.isfinite(ref).all()


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("nh,nkv", HEADS)
def test_varlen_reference_and_isolation(nh, nkv, causal):
    """flash_attention_ref on the packed batch: finite outputs and gradients, per-sequence
    independent -- with every even (odd) sequence's q|k|v and dO rows NaN, the other parity's
    outputs and gradients are unchanged."""
    qkv, do, cu = varlen_qkv(nh, nkv, torch.bfloat16, seed=2)
    assert cu[-1] == 2019 and len(cu) == len(VARLEN_LENS) + 1
    o, g = _ref_fwd_bwd(qkv, do, cu, nh, nkv, causal)
    assert torch.isfinite(o).all() and torch.isfinite(g).all()
    assert seq_err(o, o, cu) == [0.0] * len(VARLEN_LENS)
    # a 1-token sequence: softmax over one key, dq = dk = 0 up to rounding
    assert g[0, :(nh + nkv) * D].abs().max().item() < 1e-4
    for parity in (0, 1):
        o2, g2 = _ref_fwd_bwd(nan_rows(qkv, cu, parity), nan_rows(do, cu, parity), cu, nh, nkv,
                              causal)
        for s in range(len(VARLEN_LENS)):
            a, b = cu[s], cu[s + 1]
            if s % 2 == parity:
                assert o2[a:b].isnan().all()
            else:
                assert torch.equal(o2[a:b], o[a:b]) and torch.equal(g2[a:b], g[a:b])


@pytest.mark.parametrize("causal", [True, False])
def test_varlen_wide_scores(causal):
    """The wide batch: scores span roughly +-50, the boosted key gains ~+40 in every row that
    sees it, and the reference stays finite."""
    nh, nkv = 8, 2
    qkv, do, cu = varlen_qkv(nh, nkv, torch.bfloat16, seed=2, wide=True, causal=causal)
    plain, _, _ = varlen_qkv(nh, nkv, torch.bfloat16, seed=2, wide=False, causal=causal)
    assert 39 < WIDE_BOOST < 41
    s, L = len(VARLEN_LENS) - 1, VARLEN_LENS[-1]
    x = qkv[cu[s]:cu[s + 1]].float().view(L, nh + 2 * nkv, D)
    sc = torch.einsum("qd,kd->qk", x[:, 0], x[:, nh]) / math.sqrt(D)
    assert sc.max().item() > 40 and sc.min().item() < -30
    j = dominant_key(L, causal)
    rest = sc.clone()
    rest[:, j] = 0
    x0 = x.clone()
    x0[:, :, 0] = 0                              # the same scores without element 0's product
    sc0 = torch.einsum("qd,kd->qk", x0[:, 0], x0[:, nh]) / math.sqrt(D)
    assert torch.allclose(sc[:, j] - sc0[:, j], torch.full((L,), WIDE_BOOST), atol=1e-3)
    assert torch.allclose(rest, sc0.index_fill(1, torch.tensor([j]), 0), atol=1e-3)
    assert dominant_key(257, True) // 64 == 0 and dominant_key(257, False) // 64 == 4
    o, g = _ref_fwd_bwd(qkv, do, cu, nh, nkv, causal)
    assert torch.isfinite(o).all() and torch.isfinite(g).all()
    assert not torch.equal(plain, qkv)
