"""The attention kernels at their own edges, judged per sequence, over inputs where a wrong mask
or an unwritten buffer cannot hide: packed batches of lengths +-1 around every tile size with NaN
neighbours, paged caches whose every non-live slot (block 0, the last block's tail, the scratch)
is poison, ``torch.empty`` buffers that start as NaN, and scores spanning +-50.  The inputs come
from ``_attn_cases.py`` (validated on the CPU by ``test_attention_edges_cpu.py``); the references
are the project's f32 ones, the bounds those of ``test_kernels_gpu.py`` applied to every sequence
on its own.  Poison is data only -- every index stays inside its allocation."""
import functools
import math

import pytest
import torch

from _attn_cases import (BS, CHUNK_LENS, CTX_LENS, D, HEADS, KINDS, PagedCase, cu_of, nan_empty,
                         nan_rows, seq_err, varlen_qkv, wide_q)

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
FWD, GRAD, PREFILL, DECODE = 2e-2, 3e-2, 1e-2, 1e-2   # test_kernels_gpu.py's bounds


@pytest.fixture(autouse=True)
def _native():
    from lumen.ops._native import native, native_error

    assert native() is not None, f"native extension must load on the GPU box: {native_error()!r}"
    torch.manual_seed(0)


class _Worst:
    """Per-quantity maximum of seq_err over one test, printed at its end."""

    def __init__(self):
        self.w = {}

    def check(self, name, got, ref, cu, bound, only=None, what=""):
        e = seq_err(got, ref, cu)
        idx = list(range(len(e))) if only is None else list(only)
        T = int(cu[-1])
        g = got.detach().reshape(T, -1)
        for s in idx:
            assert torch.isfinite(g[cu[s]:cu[s + 1]].float()).all(), \
                f"{name} {what}: sequence {s} (rows {cu[s]}:{cu[s + 1]}) not finite"
        bad = [(s, e[s]) for s in idx if not e[s] < bound]
        self.w[name] = max(self.w.get(name, 0.0), max(e[s] for s in idx))
        assert not bad, f"{name} {what}: (sequence, seq_err) over {bound}: {bad}"

    def report(self, tag):
        print(f"{tag}: max seq_err " + " ".join(f"{k}={v:.2e}" for k, v in self.w.items()))


# ---- 1 / 2: varlen flash attention --------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _varlen_case(nh, nkv, dtype, causal, wide):
    """(qkv, dO, cu) and the f32 reference's (O, dQKV), all on the CPU, built once."""
    from lumen.ops.attention import flash_attention_ref

    qkv, do, cu = varlen_qkv(nh, nkv, dtype, seed=2, wide=wide, causal=causal)
    x = qkv.float().requires_grad_(True)
    o = flash_attention_ref(x, tuple(cu), nh, nkv, D, causal)
    (g,) = torch.autograd.grad(o, x, do.float())
    return qkv, do, cu, o.detach(), g


def _fa(qkv, do, cu, nh, nkv, causal, rope=None):
    from lumen.ops.attention import flash_attention_qkv

    x = qkv.clone().requires_grad_(True)
    o = flash_attention_qkv(x, cu, nh, nkv, D, causal, rope=rope)
    (g,) = torch.autograd.grad(o, x, do)
    return o.detach(), g


def _check_fa(w, what, o, g, ro, rg, cu, nh, nkv, only=None):
    qs, ks = nh * D, nkv * D
    w.check("O", o, ro, cu, FWD, only, what)
    w.check("dq", g[:, :qs], rg[:, :qs], cu, GRAD, only, what)
    w.check("dk", g[:, qs:qs + ks], rg[:, qs:qs + ks], cu, GRAD, only, what)
    w.check("dv", g[:, qs + ks:], rg[:, qs + ks:], cu, GRAD, only, what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("ds_mb", [2048, 0])
@pytest.mark.parametrize("nh,nkv", HEADS)
def test_varlen_edges(nh, nkv, ds_mb, causal, dtype, monkeypatch):
    """Forward and both backward paths (dS hand-off / recompute) on the packed edge lengths:
    (a) clean, (c) the same with every torch.empty buffer NaN, (b) with every other sequence's
    q|k|v and dO rows NaN -- the remaining sequences' O, dq, dk, dv keep their bounds."""
    import lumen.ops.attention as att

    monkeypatch.setattr(att, "FA_DS_MB", ds_mb)
    qkv, do, cu, ro, rg = _varlen_case(nh, nkv, dtype, causal, False)
    qkv, do = qkv.to(DEV), do.to(DEV)
    w = _Worst()
    o, g = _fa(qkv, do, cu, nh, nkv, causal)
    _check_fa(w, "clean", o, g, ro, rg, cu, nh, nkv)
    with nan_empty():
        o, g = _fa(qkv, do, cu, nh, nkv, causal)
    _check_fa(w, "nan_empty", o, g, ro, rg, cu, nh, nkv)
    for parity in (0, 1):
        with nan_empty():
            o, g = _fa(nan_rows(qkv, cu, parity), nan_rows(do, cu, parity), cu, nh, nkv, causal)
        _check_fa(w, f"NaN sequences of parity {parity}", o, g, ro, rg, cu, nh, nkv,
                  only=range(1 - parity, len(cu) - 1, 2))
    w.report(f"varlen nh={nh} nkv={nkv} ds_mb={ds_mb} causal={causal} {dtype}")


@pytest.mark.parametrize("ds_mb", [2048, 0])
def test_varlen_isolation_fused_inverse_rope(ds_mb, monkeypatch):
    """(b) through the ``rope=`` epilogues: dq / dk come back inverse-rotated, per row, and a NaN
    neighbour sequence does not leak in."""
    import lumen.ops.attention as att
    from lumen.ops.rope import _rotate_ref, rope_tables

    monkeypatch.setattr(att, "FA_DS_MB", ds_mb)
    nh, nkv, dtype = 8, 2, torch.bfloat16
    qkv, do, cu, ro, rg = _varlen_case(nh, nkv, dtype, True, False)
    T = cu[-1]
    cos, sin = rope_tables(D, 4096, 10000.0, DEV)
    pos = torch.randint(0, 4096, (T,), generator=torch.Generator().manual_seed(4)).int()
    p = pos.long()
    qk = (nh + nkv) * D
    rg = rg.clone()
    rg[:, :qk] = _rotate_ref(rg[:, :qk].view(T, nh + nkv, D), cos.cpu()[p][:, None],
                             sin.cpu()[p][:, None], inverse=True).view(T, qk)
    qkv, do, pos = qkv.to(DEV), do.to(DEV), pos.to(DEV)
    w = _Worst()
    for parity in (0, 1):
        with nan_empty():
            o, g = _fa(nan_rows(qkv, cu, parity), nan_rows(do, cu, parity), cu, nh, nkv, True,
                       rope=(pos, cos, sin))
        _check_fa(w, f"rope, NaN sequences of parity {parity}", o, g, ro, rg, cu, nh, nkv,
                  only=range(1 - parity, len(cu) - 1, 2))
    w.report(f"varlen rope ds_mb={ds_mb}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("ds_mb", [2048, 0])
@pytest.mark.parametrize("nh,nkv", HEADS)
def test_varlen_wide_scores(nh, nkv, ds_mb, causal, dtype, monkeypatch):
    """Scores spanning +-50 with one key per sequence ~40 above, in another 64-key tile than most
    rows' diagonal: the running maximum moves by tens between tiles."""
    import lumen.ops.attention as att

    monkeypatch.setattr(att, "FA_DS_MB", ds_mb)
    qkv, do, cu, ro, rg = _varlen_case(nh, nkv, dtype, causal, True)
    w = _Worst()
    o, g = _fa(qkv.to(DEV), do.to(DEV), cu, nh, nkv, causal)
    _check_fa(w, "wide", o, g, ro, rg, cu, nh, nkv)
    w.report(f"varlen wide nh={nh} nkv={nkv} ds_mb={ds_mb} causal={causal} {dtype}")


# ---- 2 / 3: paged decode ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _paged_case(kind, nkv, dtype, wide=False, bs=BS, d=D):
    return PagedCase(kind, CTX_LENS, nkv, bs, d, dtype, seed=3, wide=wide)


def _decode_all(kind, nh, nkv, dtype, wide, bs=BS, d=D):
    from lumen.ops.attention import _merge_counters, paged_decode, paged_decode_ref

    case = _paged_case(kind, nkv, dtype, wide, bs, d)
    nseq = len(CTX_LENS)
    q = torch.randn(nseq, nh, d, generator=torch.Generator().manual_seed(8)).to(dtype)
    if wide:
        q = wide_q(q).to(dtype)
    scale = 1 / math.sqrt(d)
    ref = paged_decode_ref(q.float(), case.kc, case.vc, case.bt, case.cl, scale)
    assert torch.isfinite(ref).all()
    kc, vc, bt, cl = case.to(DEV)
    q = q.to(DEV)
    cu = list(range(nseq + 1))
    w = _Worst()
    # the two-pass kernel (0) and its fused merge read 16-bit caches only
    forms = [(one, False) for one in ((0, 1, 2, 3) if kind == "16bit" else (1, 2, 3))]
    if kind == "16bit":
        forms.append((0, True))
    for part in (64, 512):
        for one, fused in forms:
            with nan_empty():
                got = paged_decode(q, kc, vc, bt, cl, max(CTX_LENS), scale, part,
                                   fused_merge=fused, one_pass=one)
            w.check(f"part{part}", got, ref, cu, DECODE,
                    what=f"one_pass={one} fused_merge={fused}")
    assert _merge_counters or kind != "16bit"   # the fused merge ran and left its counters zeroed
    assert all(int(c.abs().sum()) == 0 for c in _merge_counters.values())
    w.report(f"decode {kind} nh={nh} nkv={nkv} D={d} bs={bs} wide={wide} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("kind", KINDS)
def test_paged_decode_poisoned(kind, nh, nkv, dtype):
    """Every decode form over caches whose block 0 (the value of every unused table entry), last-
    block tails and spare blocks are poison, partials and outputs starting as NaN."""
    _decode_all(kind, nh, nkv, dtype, False)


@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("kind", KINDS)
def test_paged_decode_poisoned_d64(kind, nh, nkv):
    """D = 64 at block size 32, the shape at which the uniform-block-id forms run there (the
    pipelined one at nh == nkv only)."""
    _decode_all(kind, nh, nkv, torch.bfloat16, False, bs=32, d=64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("kind", KINDS)
def test_paged_decode_wide_scores(kind, nh, nkv, dtype):
    """Scores spanning +-50 and the last key ~40 above: where the context is split, the
    partitions' maxima differ by tens and the merge must subtract the right one."""
    _decode_all(kind, nh, nkv, dtype, True)


# ---- 4: chunked prefill -------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("kind", KINDS)
def test_chunked_prefill_poisoned(kind, nh, nkv, dtype):
    """flash_attention_paged over the poisoned caches: whole prompts, 1-row chunks around a
    64-key tile edge and a block edge, chunks ending on 128 and 512.  The fp8 / mxfp4 caches go
    through the dequantised scratch, whose every element is NaN before the call."""
    import lumen.ops.attention as att

    case = _paged_case(kind, nkv, dtype)
    cu = cu_of(CHUNK_LENS)
    g = torch.Generator().manual_seed(9)
    qr = (torch.randn(cu[-1], (nh + 2 * nkv) * D, generator=g) * 0.5).to(dtype)
    qr[:, nh * D:] = float("nan")   # the chunk's own k | v columns: the cache holds them
    ref = att.flash_attention_paged_ref(qr.float(), case.kc, case.vc, cu, CTX_LENS, case.bt, nh,
                                        nkv, D)
    assert torch.isfinite(ref).all()
    kc, vc, bt, _ = case.to(DEV)
    qr = qr.to(DEV)
    w = _Worst()
    with nan_empty():
        got = att.flash_attention_paged(qr, kc, vc, cu, CTX_LENS, bt, nh, nkv, D)
    w.check("O", got, ref, cu, PREFILL, what="nan_empty")
    if kind != "16bit":
        scr = [v for k, v in att._SCRATCH.items() if k[1:] == (dtype, nkv, BS, D)]
        assert len(scr) == 1, list(att._SCRATCH)
        scr[0][0].fill_(float("nan"))
        scr[0][1].fill_(float("nan"))
        with nan_empty():
            got = att.flash_attention_paged(qr, kc, vc, cu, CTX_LENS, bt, nh, nkv, D)
        w.check("O", got, ref, cu, PREFILL, what="NaN scratch")
        assert any(k[1:] == (dtype, nkv, BS, D) and v is scr[0] for k, v in att._SCRATCH.items())
    w.report(f"prefill {kind} nh={nh} nkv={nkv} {dtype}")


# ---- 5: the cache-write kernels leave the rest alone --------------------------------------------

def _noise_cache(kind, nblocks, nkv, dtype, g):
    """A cache of random bytes (NaN patterns included) and its byte view."""
    from lumen.ops.attention import FP8_KV

    ct = FP8_KV if kind == "fp8" else dtype
    esz = 1 if kind == "fp8" else 2
    raw = torch.randint(0, 256, (nblocks, nkv, BS, D * esz), generator=g, dtype=torch.uint8)
    raw = raw.to(DEV)
    return raw.view(ct), raw


def _check_written(cache_raw, before, slots, rows, kind, dtype, min_equal):
    """Bytes outside the slots unchanged; the slots hold ``rows`` [T, nkv, D] (16-bit: the same
    bits; fp8: torch's e4m3fn cast, up to the share the fp8 cache test allows)."""
    from lumen.ops.attention import FP8_KV

    ok = slots >= 0
    blk, off = slots[ok] // BS, slots[ok] % BS
    keep = torch.ones(before.shape[0], BS, dtype=torch.bool, device=DEV)
    keep[blk, off] = False
    assert int(keep.sum()) == keep.numel() - int(ok.sum()) < keep.numel() - 30
    keep = keep[:, None, :, None].expand_as(before)
    assert torch.equal(cache_raw[keep], before[keep]), "bytes outside the written slots changed"
    got = cache_raw[blk, :, off]
    if kind == "fp8":
        want = rows[ok].contiguous().to(FP8_KV).view(torch.uint8)
        assert (got == want).float().mean().item() > min_equal
    else:
        want = rows[ok].contiguous().view(torch.uint8).view(got.shape)
        assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("kind", ["16bit", "fp8"])
def test_cache_writes_leave_the_rest_alone(kind, nh, nkv, dtype):
    """write_kv_cache and rope_write_kv into caches of random bytes, scattered slots with some
    -1: every byte outside the written slots is unchanged.  (The mxfp4 cache has this test in
    test_kv_mxfp4_gpu.)"""
    from lumen.ops.attention import rope_write_kv, write_kv_cache
    from lumen.ops.rope import _rotate_ref, rope_tables

    g = torch.Generator().manual_seed(6)
    T, nblocks = 45, 9
    slots = torch.randperm(nblocks * BS, generator=g)[:T]
    slots[torch.tensor([0, 4, 20, T - 1])] = -1
    slots = slots.to(DEV)
    # strided rows, as the engine's views into the fused qkv buffer are
    kv = (torch.randn(T, 2 * nkv, D, generator=g) * 3).to(dtype).to(DEV)
    (kc, kraw), (vc, vraw) = (_noise_cache(kind, nblocks, nkv, dtype, g) for _ in range(2))
    k0, v0 = kraw.clone(), vraw.clone()
    write_kv_cache(kv[:, :nkv], kv[:, nkv:], kc, vc, slots)
    _check_written(kraw, k0, slots, kv[:, :nkv], kind, dtype, 0.999)
    _check_written(vraw, v0, slots, kv[:, nkv:], kind, dtype, 0.999)

    qkv = torch.randn(T, (nh + 2 * nkv) * D, generator=g).to(dtype).to(DEV)
    pos = torch.randint(0, 400, (T,), generator=g).int().to(DEV)
    cos, sin = rope_tables(D, 4096, 10000.0, DEV)
    (kc, kraw), (vc, vraw) = (_noise_cache(kind, nblocks, nkv, dtype, g) for _ in range(2))
    k0, v0 = kraw.clone(), vraw.clone()
    kr = qkv[:, nh * D:(nh + nkv) * D].reshape(T, nkv, D)
    p = pos.long()
    k32 = _rotate_ref(kr.float(), cos[p][:, None], sin[p][:, None])
    rope_write_kv(qkv, pos, nh, nkv, D, cos, sin, kc, vc, slots)
    # a 16-bit cache holds the rotated k as written back to the qkv rows, bit for bit; an fp8 one
    # the e4m3fn cast of the f32 rotation (against the cast of the 16-bit rows, 1 element in 32
    # differs: the 16-bit rounding lands on an fp8 tie in 1 of 16 and breaks it the other way in
    # half of those -- measured 3.4 %); v is stored as it is
    if kind != "fp8":
        k32 = qkv[:, nh * D:(nh + nkv) * D].reshape(T, nkv, D)
    vr = qkv[:, (nh + nkv) * D:].reshape(T, nkv, D)
    _check_written(kraw, k0, slots, k32, kind, dtype, 0.999)
    _check_written(vraw, v0, slots, vr, kind, dtype, 0.999)
