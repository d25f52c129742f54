"""Inputs of the attention edge tests (``test_attention_edges_cpu.py`` / ``_gpu.py``): packed
batches at the kernels' tile edges, paged caches whose every non-live byte is poison, wide score
ranges, a per-sequence error metric and a ``torch.empty`` that hands out NaN.

Everything is built on the CPU through the torch definitions (``Mxfp4KV.write``, the CPU path of
``write_kv_cache``), so the attention tests do not lean on the cache-write kernels and the CPU
test validates exactly the data the GPU tests run on.  Poison is data only: every block id, slot
and length stays inside its allocation.
"""
from __future__ import annotations

import contextlib
import math
from typing import List, Sequence

import torch

from lumen.ops.attention import FP8_KV, Mxfp4KV

# +-1 around 32 rows a wave, 64-key tiles, 128-query tiles and the `q0 + 64 < L` second Q image
VARLEN_LENS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257]
# +-1 around the KV block (16), the decode step (64 rows of a 16-bit cache, 128 of an fp8 / mxfp4
# one at D = 128) and the partition sizes 64 and 512
CTX_LENS = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1025]
# chunk lengths paired with CTX_LENS as kv_lens: whole prompts, 1-row chunks just before / after
# a 64-key tile edge and a block edge, chunks ending exactly on 128 and 512
CHUNK_LENS = [1, 1, 16, 1, 63, 64, 1, 127, 28, 129, 12, 512, 13, 100, 129]
HEADS = [(8, 2), (4, 4)]
KINDS = ["16bit", "fp8", "mxfp4"]
D, BS = 128, 16

assert sum(VARLEN_LENS) == 2019 and sum(CHUNK_LENS) == 1197
assert all(n <= L for n, L in zip(CHUNK_LENS, CTX_LENS))


def cu_of(lens: Sequence[int]) -> List[int]:
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + int(n))
    return cu


def seq_err(got: torch.Tensor, ref: torch.Tensor, cu: Sequence[int]) -> List[float]:
    """Per sequence s (rows cu[s]:cu[s+1]): ||got_s - ref_s||_F / max(||ref_s||_F,
    sqrt(n_s / T) ||ref||_F).  The floor is the batch's RMS row norm scaled to the sequence's row
    count, so an exactly-zero reference (dq / dk of a 1-token sequence) is judged against a typical
    row instead of being divided by ~0.  A non-finite ``got`` row gives nan or inf (never passes a
    ``<`` bound).  Decode: one row per sequence, ``cu = range(nseq + 1)``."""
    T = int(cu[-1])
    g = got.detach().double().reshape(T, -1)
    r = ref.detach().to(g.device).double().reshape(T, -1)
    tot = r.norm().item()
    out = []
    for s in range(len(cu) - 1):
        a, b = int(cu[s]), int(cu[s + 1])
        den = max(r[a:b].norm().item(), math.sqrt((b - a) / T) * tot)
        out.append(((g[a:b] - r[a:b]).norm() / den).item())
    return out


# ---- poisoned paged caches ----------------------------------------------------------------------

def poisoned_cache(kind: str, nblocks: int, nkv: int, bs: int, D: int, dtype, device="cpu"):
    """A cache whose every byte is poison: NaN (16-bit), 0x7F = the e4m3fn NaN (fp8), codes 0x77
    under scale bytes 0xFF = the E8M0 NaN (mxfp4)."""
    if kind == "16bit":
        return torch.full((nblocks, nkv, bs, D), float("nan"), dtype=dtype, device=device)
    if kind == "fp8":
        return torch.full((nblocks, nkv, bs, D), 0x7F, dtype=torch.uint8,
                          device=device).view(FP8_KV)
    assert kind == "mxfp4", kind
    c = Mxfp4KV(nblocks, nkv, bs, D, device)
    c.buf.fill_(0x77)
    c.scale.fill_(0xFF)
    return c


def cache_write_ref(cache, rows: torch.Tensor, blk: torch.Tensor, off: torch.Tensor) -> None:
    """rows [n, nkv, D] -> slots (blk[i], off[i]): the torch definition of the cache write."""
    if isinstance(cache, Mxfp4KV):
        cache.write(rows, blk, off)
    else:
        cache[blk, :, off] = rows.to(cache.dtype)


def cache_f32(cache) -> torch.Tensor:
    return cache.dequant_f32() if isinstance(cache, Mxfp4KV) else cache.float()


def cache_to(cache, device):
    if isinstance(cache, Mxfp4KV):
        nb, nkv, bs, D = cache.shape
        c = Mxfp4KV(nb, nkv, bs, D, device)
        c.buf.copy_(cache.buf)
        return c
    if cache.dtype == FP8_KV:
        return cache.view(torch.uint8).to(device).view(FP8_KV)
    return cache.to(device)


def poison_share(cache) -> float:
    """Share of the dequantised cache that is not finite."""
    return 1.0 - torch.isfinite(cache_f32(cache)).float().mean().item()


def block_table(lens: Sequence[int], bs: int, seed: int, spare: int = 3):
    """([nseq, maxb] int32 table, nblocks).  Live entries: a shuffled permutation of blocks 1..;
    block 0 stays entirely poison and is the value of every unused entry (the engine pads its
    tables with 0); ``spare`` further blocks are never referenced."""
    nblk = [(int(L) + bs - 1) // bs for L in lens]
    live = sum(nblk)
    perm = (torch.randperm(live, generator=torch.Generator().manual_seed(seed)) + 1).int()
    bt = torch.zeros(len(lens), max(nblk), dtype=torch.int32)
    used = 0
    for i, n in enumerate(nblk):
        bt[i, :n] = perm[used:used + n]
        used += n
    return bt, live + 1 + spare


class PagedCase:
    """K / V caches of ``kind`` over ``lens`` tokens a sequence, every other slot poison."""

    def __init__(self, kind, lens, nkv, bs, D, dtype, seed=0, wide=False):
        g = torch.Generator().manual_seed(seed)
        self.kind, self.lens, self.bs = kind, [int(x) for x in lens], bs
        self.bt, nblocks = block_table(lens, bs, seed + 1)
        self.kc = poisoned_cache(kind, nblocks, nkv, bs, D, dtype)
        self.vc = poisoned_cache(kind, nblocks, nkv, bs, D, dtype)
        for i, L in enumerate(self.lens):
            k = (torch.randn(L, nkv, D, generator=g) * (3.0 if not wide else 1.0)).to(dtype)
            v = torch.randn(L, nkv, D, generator=g).to(dtype)
            if wide:  # element 0 of the LAST key's head rows carries the dominant score (below)
                k[:, :, 0] = 0
                k[L - 1, :, 0] = WIDE_K0
            t = torch.arange(L)
            blk, off = self.bt[i, t // bs].long(), t % bs
            cache_write_ref(self.kc, k, blk, off)
            cache_write_ref(self.vc, v, blk, off)
        self.cl = torch.tensor(self.lens, dtype=torch.int32)

    def to(self, device):
        return cache_to(self.kc, device), cache_to(self.vc, device), self.bt.to(device), \
            self.cl.to(device)


# ---- wide score ranges --------------------------------------------------------------------------
# q rows of standard deviation 12 against k rows of standard deviation 1 (paged), or 24 against 0.5
# (packed qkv), give scores of standard deviation 12: the extremes over the batch's (row, key)
# pairs span roughly +-50.  On top, element 0 of every q head is WIDE_Q0 and element 0 of ONE key
# row of every sequence WIDE_K0 (0 in the others): that key's score gains
# WIDE_Q0 * WIDE_K0 / sqrt(128) = +40 in every row.  Both are exact in bf16, fp16 and e4m3.
WIDE_Q0, WIDE_K0 = 16.0, 28.0
WIDE_BOOST = WIDE_Q0 * WIDE_K0 / math.sqrt(128)


def dominant_key(L: int, causal: bool) -> int:
    """The boosted key of a packed sequence.  Causal: key min(3, L - 1), in the first 64-key tile,
    so every row from the second tile on meets the maximum first and its diagonal tile, tens
    lower, last; non-causal: the last key, so every row rescales its running state by ~e^-40 in
    its last tile.  (Paged caches boost the last key: it lies in the last partition, so the
    partition maxima differ by tens wherever there is more than one.)"""
    return min(3, L - 1) if causal else L - 1


def varlen_qkv(nh, nkv, dtype, seed=0, wide=False, causal=True, lens=VARLEN_LENS):
    """(qkv [T, (nh + 2 nkv) D], dO [T, nh D], cu) of the packed batch, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    cu = cu_of(lens)
    T = cu[-1]
    qkv = torch.randn(T, (nh + 2 * nkv) * D, generator=g) * 0.5
    if wide:
        x = qkv.view(T, nh + 2 * nkv, D)
        x[:, :nh] *= 48.0                       # score std 0.5 * 24 = 12
        x[:, :nh, 0] = WIDE_Q0
        x[:, nh:nh + nkv, 0] = 0
        for s, L in enumerate(lens):
            x[cu[s] + dominant_key(L, causal), nh:nh + nkv, 0] = WIDE_K0
    do = torch.randn(T, nh * D, generator=g)
    return qkv.to(dtype), do.to(dtype), cu


def wide_q(q: torch.Tensor) -> torch.Tensor:
    """Decode / prefill q rows [..., nh, D] for a ``wide`` PagedCase (k of standard deviation 1)."""
    q = q.float() * 12.0
    q[..., 0] = WIDE_Q0
    return q


def nan_rows(x: torch.Tensor, cu: Sequence[int], parity: int) -> torch.Tensor:
    """A copy of x with the rows of every sequence s, s % 2 == parity, set to NaN."""
    x = x.clone()
    for s in range(parity, len(cu) - 1, 2):
        x[cu[s]:cu[s + 1]] = float("nan")
    return x


# ---- torch.empty that hands out poison ----------------------------------------------------------

def _poison_(t: torch.Tensor) -> torch.Tensor:
    if t.numel() == 0:
        return t
    if t.element_size() == 1 and (t.dtype == torch.uint8 or t.is_floating_point()):
        t.view(torch.uint8).fill_(0x7F)
    elif t.is_floating_point():
        t.fill_(float("nan"))
    return t


@contextlib.contextmanager
def nan_empty():
    """For the duration of one call under test, ``torch.empty`` / ``torch.empty_like`` return
    NaN-filled floating tensors and 0x7F-filled fp8 / uint8 tensors: an output row that is never
    written, or any read of an unwritten lse / delta / dS / partial / scratch element, shows."""
    empty, empty_like = torch.empty, torch.empty_like

    def _empty(*a, **k):
        return _poison_(empty(*a, **k))

    def _empty_like(*a, **k):
        return _poison_(empty_like(*a, **k))

    torch.empty, torch.empty_like = _empty, _empty_like
    try:
        yield
    finally:
        torch.empty, torch.empty_like = empty, empty_like
