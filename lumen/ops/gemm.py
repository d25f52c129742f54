"""Projection GEMMs: y = x @ W^T, ``linear_nt`` choosing the route by weight type and M.

16-bit weights.  At decode batch 1-4 the projection is a pure stream of the weight matrix; for
the shapes where it measured faster the HIP weight-streaming kernel (``kernels/skinny_gemm.hip``)
runs it instead of a library GEMM.  Batches 5..256 take the decode-batch MFMA kernel
(``kernels/decode_gemm.hip``) where its plan table lists the shape.  Everything else (and CPU
tensors) goes to ``torch.matmul`` (hipBLASLt with the tuned table), ``mm_nt`` splitting
training-size outputs at the last whole wave of tiles.

Quantized weights (ops/quant.py), each with a GEMV for M <= 4 and / or a decode MFMA kernel for
M <= 256 behind a measured plan table, and a fallback that dequantises W into a persistent 16-bit
scratch and takes the 16-bit path:

* ``QuantWeight``, act None (``fp8``)     -> ``_linear_w8``    kernels/w8_gemm.hip
* ``QuantWeight``, act "fp8" (``ptpc_fp8``) -> ``_linear_w8a8``  kernels/w8a8_gemm.hip (+ M > 256)
* ``Mxfp4Weight``, act "fp8" (``mxfp4``)   -> ``_linear_w4a8``  kernels/w4a8_gemm.hip
* ``Mxfp4Weight``, act None (``mxfp4_a16``) -> ``_linear_w4a16`` kernels/w4a16_gemm.hip

The five decode MFMA kernels share one split-K workspace per (device, stream) (``_dg_splitk_ws``;
the contract is in ``kernels/dgemm.h``), the plan files one format (``load_plans``) and one place
(``configs/kernels/``, each with an environment override)."""
from __future__ import annotations

import os
from typing import Optional

import torch

from ._native import native, use_native
from .quant import Mxfp4Weight, QuantWeight

# Measured per shape against hipBLASLt with the tuned table (lumen/bench/skinny_bench.py
# --m1-forms, profiles/r02_serve/m1_forms.jsonl): the rows-per-lane weight-streaming kernel
# reaches 4.3-6.5 TB/s at M = 1 and beats hipBLASLt at every Llama-2-7B projection (qkv 17.0 vs
# 22.9 us, o 7.8 vs 22.7, gate_up 27.8 vs 37.3, down 16.5 vs 27.5, lm_head 38.4 vs 60.6); at
# M = 2 it still wins or ties everywhere (o 10.4 vs 22.6, down 20.7 vs 27.6, lm_head 51.4 vs
# 59.0); at M = 3-4 only the N = 4096 projections (o, down) stay ahead, and from M = 5 on
# hipBLASLt wins, so those are library GEMMs.
SKINNY_MAX_M = int(os.environ.get("LUMEN_SKINNY_MAX_M", "4"))
SKINNY_MAX_N = int(os.environ.get("LUMEN_SKINNY_MAX_N", str(1 << 30)))
SKINNY_WIDE_MAX_M = 2  # above this M only N <= 4096 projections take the GEMV


def skinny_ok(x: torch.Tensor, w: torch.Tensor) -> bool:
    return (0 < x.shape[0] <= min(SKINNY_MAX_M, 16) and w.shape[0] <= SKINNY_MAX_N
            and (x.shape[0] <= SKINNY_WIDE_MAX_M or w.shape[0] <= 4096)
            and use_native(x) and x.dim() == 2
            and w.dim() == 2 and x.dtype == w.dtype and x.dtype in (torch.bfloat16, torch.float16)
            and x.stride(1) == 1 and w.is_contiguous() and x.shape[1] == w.shape[1]
            and (w.shape[0] % 4 == 0 and w.shape[1] % 8 == 0 and x.stride(0) % 8 == 0
                 if x.shape[0] <= 4 else w.shape[0] % 16 == 0 and w.shape[1] % 128 == 0))


# Decode batches 5..256: the decode-batch MFMA GEMM (kernels/decode_gemm.hip) where the measured
# plan table (configs/kernels/decode_gemm_plans.json, written by lumen/bench/decode_gemm_probe.py) has
# a winning (BM, BN, split-K) for the shape, hipBLASLt with the tuned table otherwise.  (Two
# earlier hand-written attempts lost, scripts/probes/: 32-row M tiles, and all-M-rows tiles over
# all of K whose every workgroup pulled the whole x through its CU's load path.)
DG_BMS = (64, 128, 192, 256)
DG_BNS = {256: (64, 96, 128, 160), 192: (64, 96, 128), 128: (64, 96, 128, 192, 256),
          64: (64, 128, 192, 256)}
DG_BNS8 = {256: (64, 128), 128: (128, 256)}   # 8-wave variants
DGEMM = os.environ.get("LUMEN_DGEMM", "1") != "0"
_dg_ws: dict = {}
_dg_old: list = []
_dg_plans: Optional[dict] = None


def dg_bucket(M: int) -> int:
    return next(b for b in DG_BMS if M <= b)


def _y(rows: int, w, like: torch.Tensor, out: Optional[torch.Tensor],
       dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``out``, or a new [rows, N] result on ``like``'s device, of ``dtype`` (``like``'s where
    none is given; the act-fp8 routes pass the weight's, their ``like`` being the fp8 xq)."""
    if out is not None:
        return out
    return torch.empty(rows, w.shape[0], device=like.device, dtype=dtype or like.dtype)


def decode_gemm(x: torch.Tensor, w: torch.Tensor, bm: int, bn: int, s: int, nw: int = 4,
                out: Optional[torch.Tensor] = None, flags: int = 0,
                m: Optional[int] = None) -> torch.Tensor:
    """y = x @ w^T on the decode-batch MFMA kernel with block tile (bm, bn), split-K s and nw
    (4 or 8) waves per block.  ``flags``: bit 0 rotates each tile's k loop start; bit 1 takes
    x in the k-tiled layout [K / 64, bm, 64] (``x_ktiled``) with ``m`` valid rows."""
    y = _y(x.shape[0] if not flags & 2 else int(m), w, x, out)
    ws, cnt = _dg_splitk_ws(x.device, w.shape[0], bm, bn, s)
    native().decode_gemm(x, w, y, ws, cnt, bm, bn, s, nw, flags)
    return y


def _dg_splitk_ws(device, N: int, bm: int, bn: int, s: int) -> tuple:
    """(slab workspace, ticket counters) for a split-K launch of ``s`` slices over [bm, bn]
    tiles of N columns on the current stream; (None, None) for s == 1.  Shared by the 16-bit and
    the four quantized decode GEMMs: launches on one stream run one after the other, and every
    launch leaves the counters zero (kernels/dgemm.h)."""
    if s <= 1:
        return None, None
    # one slab workspace + ticket counters per (device, stream): split-K slabs and tickets
    # of GEMMs on different streams never interleave (a side-stream GEMM gets its own)
    key = _dg_key(device)
    got = _dg_ws.get(key)
    need = -(-N // bn) * s * bm * bn
    if got is None or got[0].numel() < need or got[1].numel() < -(-N // bn):
        # generous size; a superseded pair stays alive (_dg_old): a captured decode graph
        # keeps pointing at the buffers it was captured with
        n = max(need, 1 << 24)
        if got is not None:
            _dg_old.append(got)
        got = (torch.empty(n, dtype=torch.float32, device=device),
               torch.zeros(max(4096, -(-N // bn)), dtype=torch.int32, device=device))
        _dg_ws[key] = got
    return got


def x_ktiled(x: torch.Tensor, bm: int = 256) -> torch.Tensor:
    """[M, K] -> [K / 64, bm, 64] (rows past M zero): the decode GEMM's k-tiled x layout."""
    M, K = x.shape
    t = torch.zeros(K // 64, bm, 64, device=x.device, dtype=x.dtype)
    t[:, :M].copy_(x.reshape(M, K // 64, 64).transpose(0, 1))
    return t


def _dg_key(device) -> tuple:
    return (str(device), torch.cuda.current_stream(device).cuda_stream)


def dg_workspace(device) -> Optional[tuple]:
    """(slab workspace, ticket counters) of the current stream on ``device`` (None before the
    first split-K call there)."""
    return _dg_ws.get(_dg_key(device))


def load_plans(path: str, with_nw: bool = False) -> dict:
    """{(N, K, BM): (BN, S)} from a plan file ({"plans": [{"N", "K", "BM", "BN", "S"}, ...]});
    {} for a missing file.  ``with_nw``: (BN, S, waves) -- the 16-bit table's ``NW``, 4 where an
    entry omits it.  For the W8A8 table a ``BM`` above 256 is an M bucket of the large-M kernel
    (``W8A8_GEMM_BUCKETS``), whose block tile is fixed."""
    import json

    plans = {}
    if os.path.exists(path):
        with open(path) as f:
            for e in json.load(f).get("plans", []):
                nw = (e.get("NW", 4),) if with_nw else ()
                plans[(e["N"], e["K"], e["BM"])] = (e["BN"], e["S"]) + nw
    return plans


load_w8_plans = load_w8a8_plans = load_w4a8_plans = load_w4a16_plans = load_plans


def _plan_path(env: str, name: str) -> str:
    """The plan file named by the environment variable ``env``, else the shipped table
    configs/kernels/``name`` (measured wins over the route's fallback only)."""
    return os.environ.get(env, os.path.join(
        os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
        "configs", "kernels", name))


def dg_plans() -> dict:
    """{(N, K, BM): (BN, S, waves)} of the 16-bit decode GEMM."""
    global _dg_plans
    if _dg_plans is None:
        _dg_plans = load_plans(_plan_path("LUMEN_DGEMM_PLANS", "decode_gemm_plans.json"),
                               with_nw=True)
    return _dg_plans


def dg_plan(x: torch.Tensor, w: torch.Tensor) -> Optional[tuple]:
    if not (DGEMM and use_native(x) and x.dim() == 2 and w.dim() == 2 and 4 < x.shape[0] <= 256
            and x.dtype == w.dtype and x.dtype in (torch.bfloat16, torch.float16)
            and x.stride(1) == 1 and x.stride(0) % 8 == 0 and w.is_contiguous()
            and x.shape[1] == w.shape[1] and w.shape[1] % 64 == 0 and w.shape[0] % 4 == 0):
        return None
    bm = dg_bucket(x.shape[0])
    p = dg_plans().get((w.shape[0], w.shape[1], bm))
    return (bm,) + tuple(p) if p is not None else None


# Training-shape GEMMs run 256 x 256 macro tiles, one per CU at a time, so a GEMM with 5.375 or
# 2.69 waves of tiles on the 256-CU chip takes 6 or 3 waves (Llama-2-7B at T = 4096: gate|up
# forward 16 x 86 tiles, down input-grad 16 x 43).  ``mm_nt`` splits the output columns at the
# last whole wave and runs the remainder as its own (separately tuned) GEMM, both writing column
# views of one buffer (ldc = full width, no copies).  scripts/probes/split_gemm_probe.py measures it.
GEMM_SPLIT = os.environ.get("LUMEN_GEMM_SPLIT", "1") != "0"
SPLIT_TILE, SPLIT_CUS = 256, 256
SPLIT_MAX_TAIL = float(os.environ.get("LUMEN_GEMM_SPLIT_MAX_TAIL", "0.75"))


def split_cols(M: int, N: int) -> int:
    """Column count of the whole-wave part of an [M, N] output (0: no split).  Splits only when
    the last wave is at most ``SPLIT_MAX_TAIL`` full and the wave boundary is a column-tile
    boundary."""
    if M % SPLIT_TILE or N % 8:
        return 0
    tm, tn = M // SPLIT_TILE, -(-N // SPLIT_TILE)
    total = tm * tn
    waves, tail = divmod(total, SPLIT_CUS)
    if waves == 0 or tail == 0 or tail > SPLIT_MAX_TAIL * SPLIT_CUS or SPLIT_CUS % tm:
        return 0
    n1 = waves * (SPLIT_CUS // tm) * SPLIT_TILE
    return n1 if 0 < n1 < N else 0


_tuned: dict = {"n": -1, "sigs": frozenset()}


def _tuned_sigs() -> frozenset:
    """Problem signatures of the loaded TunableOp table (refreshed when its size changes)."""
    try:
        import torch.cuda.tunable as tn

        if not tn.is_enabled():
            return frozenset()
        res = tn.get_results()
    except Exception:  # noqa: BLE001
        return frozenset()
    if len(res) != _tuned["n"]:
        _tuned["n"], _tuned["sigs"] = len(res), frozenset(r[1] for r in res)
    return _tuned["sigs"]


def _split_plan(x: torch.Tensor, w: torch.Tensor) -> int:
    if not (GEMM_SPLIT and x.is_cuda and x.dim() == 2 and w.dim() == 2 and x.stride(1) == 1
            and w.stride(1) == 1):
        return 0
    (M, K), N = x.shape, w.shape[0]
    n1 = split_cols(M, N)
    if not n1:
        return 0
    # only where both parts have tuned solutions (untuned shapes would fall to the heuristic);
    # decided once per problem (the table is loaded before the first training GEMM)
    key = (M, N, K, w.stride(0), x.stride(0))
    hit = _plans.get(key)
    if hit is None:
        sigs = _tuned_sigs()
        lds = f"ld_{w.stride(0)}_{x.stride(0)}_{N}"
        hit = n1 if (f"tn_{n1}_{M}_{K}_{lds}" in sigs
                     and f"tn_{N - n1}_{M}_{K}_{lds}" in sigs) else 0
        _plans[key] = hit
    return hit


_plans: dict = {}


def mm_nt(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """x [M, K] @ w[N, K]^T -> [M, N] (w row-contiguous), split at the last whole wave of tiles
    on the GPU (see ``split_cols``)."""
    n1 = _split_plan(x, w)
    if not n1:
        return torch.matmul(x, w.t())
    y = torch.empty(x.shape[0], w.shape[0], device=x.device, dtype=torch.result_type(x, w))
    torch.mm(x, w[:n1].t(), out=y[:, :n1])
    torch.mm(x, w[n1:].t(), out=y[:, n1:])
    return y


# ---- fp8 weight-only projections (ops/quant.py QuantWeight, kernels/w8_gemm.hip) ---------------
# M <= 4: the fp8 rows-per-lane GEMV at every N (the weight stream is the cost at every N);
# 5 <= M <= 256: the W8A16 MFMA kernel where the measured plan table
# (configs/kernels/w8_gemm_plans.json, derived from profiles/w8_serve) lists the shape; everything
# else -- prefill / mixed steps, shapes the kernels refuse -- dequantises into a persistent 16-bit
# scratch (w8_dequant) and takes the 16-bit path above unchanged (same GEMM shapes and leading
# dimensions, so the TunableOp table still applies).  LUMEN_W8=0 forces that fallback everywhere.
W8 = os.environ.get("LUMEN_W8", "1") != "0"
W8_BMS = (64, 128, 256)
W8_BNS = {64: (64, 128), 128: (64, 128), 256: (64,)}   # compiled (BM, BN) variants
_w8_plans: Optional[dict] = None
_w8_scratch: dict = {}
_w8_old: list = []
_w8_reserved: dict = {}


def w8_plans() -> dict:
    """{(N, K, BM): (BN, S)} of the W8A16 decode GEMM."""
    global _w8_plans
    if _w8_plans is None:
        _w8_plans = load_plans(_plan_path("LUMEN_W8_PLANS", "w8_gemm_plans.json"))
    return _w8_plans


def _w8_common_ok(x: torch.Tensor, w) -> bool:
    return (x.dim() == 2 and x.dtype == w.dtype and x.dtype in (torch.bfloat16, torch.float16)
            and x.stride(1) == 1 and x.stride(0) % 8 == 0 and x.stride(0) >= w.shape[1]
            and x.shape[1] == w.shape[1] and w.q.is_contiguous() and w.shape[0] % 4 == 0 and x.data_ptr() % 16 == 0)


def w8_gemv_ok(x: torch.Tensor, w) -> bool:
    return 0 < x.shape[0] <= 4 and _w8_common_ok(x, w) and w.shape[1] % 16 == 0


def w8_plan(x: torch.Tensor, w) -> Optional[tuple]:
    """(BM, BN, S) of the MFMA kernel for this call, None where it does not apply."""
    if not (4 < x.shape[0] <= 256 and _w8_common_ok(x, w) and w.shape[1] % 64 == 0
            and w.scale.data_ptr() % 16 == 0):
        return None
    bm = next(b for b in W8_BMS if x.shape[0] <= b)
    p = w8_plans().get((w.shape[0], w.shape[1], bm))
    return (bm,) + tuple(p) if p is not None else None


def w8_decode_gemm(x: torch.Tensor, w, bm: int, bn: int, s: int,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x @ (w.q * w.scale[:, None])^T on the W8A16 MFMA kernel with block tile (bm, bn) and
    split-K s."""
    y = _y(x.shape[0], w, x, out)
    ws, cnt = _dg_splitk_ws(x.device, w.shape[0], bm, bn, s)
    native().w8_decode_gemm(x, w.q, w.scale, y, ws, cnt, bm, bn, s)
    return y


def w8_reserve(device, numel: int) -> None:
    """Size every later dequant scratch on ``device`` for at least ``numel`` elements (the
    largest projection being served), so a scratch never grows after a decode graph captured
    it."""
    _w8_reserved[str(device)] = max(_w8_reserved.get(str(device), 0), int(numel))


def _scratch16(w) -> torch.Tensor:
    """The [N, K] view for ``w`` of the persistent 16-bit scratch of the current (device, stream)
    and ``w.dtype``, grown where needed (never below ``w8_reserve``'s floor)."""
    N, K = w.shape
    key = _dg_key(w.device) + (w.dtype,)
    buf = _w8_scratch.get(key)
    if buf is None or buf.numel() < N * K:
        # a superseded scratch stays alive (_w8_old): a captured graph keeps pointing at it
        if buf is not None:
            _w8_old.append(buf)
        buf = torch.empty(max(N * K, _w8_reserved.get(str(w.device), 0)), dtype=w.dtype,
                          device=w.device)
        _w8_scratch[key] = buf
    return buf[:N * K].view(N, K)


def w8_dequant(w, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The 16-bit weight of ``w`` (bit-identical to ``w.dequant()``), by default in the
    persistent scratch of the current (device, stream): valid until the next call there."""
    N, K = w.shape
    if K % 16:
        raise ValueError(f"fp8 weights on the GPU need K % 16 == 0, got K = {K}")
    if out is None:
        out = _scratch16(w)
    native().w8_dequant(w.q, w.scale, out)
    return out


# ---- fp8 activations x fp8 weights (QuantWeight.act == "fp8", kernels/w8a8_gemm.hip) -----------
# Every route computes ops/quant.py's one function: the activation-quant kernel once, then by M
# the W8A8 GEMV (M <= 4), the decode MFMA kernel (5..256) or the block-tiled kernel (M > 256)
# where the measured plan table (configs/kernels/w8a8_gemm_plans.json, derived from
# profiles/w8a8_serve by lumen/bench/w8a8_bench.py) lists the bucket; everything else is the
# fake-quant fallback: xq widened exactly to 16 bits, W dequantised into the weight-only path's
# scratch, the 16-bit path, and the rows multiplied by sx.  LUMEN_W8=0 forces that fallback.
W8A8_BMS = W8_BMS
W8A8_BNS = {64: (64, 128), 128: (64, 128, 256), 256: (64, 128)}   # compiled (BM, BN) variants
W8A8_FORMS = (0, 1)                     # 0: scaled K = 128 MFMA, 1: non-scaled K = 32 MFMA
# measured (profiles/w8a8_serve): the decode kernel is bound by the weight stream and its x
# staging, not by the matrix cores, and the two forms are within 1-3 % of each other at every
# shape; summed over the best candidates of all 5 <= M <= 256 rows the non-scaled form is ahead
# (1116 vs 1129 us), so it is the default and the plan table is derived for it
W8A8_FORM = int(os.environ.get("LUMEN_W8A8_FORM", "1"))
W8A8_GEMM_TILES = ((128, 128),)         # compiled block tiles of the large-M kernel
W8A8_GEMM_BUCKETS = (512, 2048, 4096)   # M buckets of the large-M plans (the last: every M above)
_w8a8_plans: Optional[dict] = None


def w8a8_plans() -> dict:
    """{(N, K, BM): (BN, S)} of the W8A8 kernels (BM above 256: a large-M kernel bucket)."""
    global _w8a8_plans
    if _w8a8_plans is None:
        _w8a8_plans = load_plans(_plan_path("LUMEN_W8A8_PLANS", "w8a8_gemm_plans.json"))
    return _w8a8_plans


def w8a8_gemm_bucket(M: int) -> int:
    return next((b for b in W8A8_GEMM_BUCKETS if M <= b), W8A8_GEMM_BUCKETS[-1])


def w8a8_plan(M: int, w) -> Optional[tuple]:
    """(BM, BN, S) of the decode kernel for 5 <= M <= 256, (bucket, BN, S) of the large-M kernel
    for M > 256; None where the table does not list the bucket."""
    if M <= 4 or w.shape[0] % 4 or w.scale.data_ptr() % 16:
        return None
    bm = next(b for b in W8A8_BMS if M <= b) if M <= 256 else w8a8_gemm_bucket(M)
    p = w8a8_plans().get((w.shape[0], w.shape[1], bm))
    return (bm,) + tuple(p) if p is not None else None


def act_quant_fp8(x: torch.Tensor) -> tuple:
    """(xq [M, K] e4m3fn, sx [M] f32) of 16-bit ``x`` on the GPU, bit-identical to
    ``ops.quant.quantize_fp8_tokens``."""
    M, K = x.shape
    if K % 16:
        raise ValueError(f"fp8 activations on the GPU need K % 16 == 0, got K = {K}")
    if x.stride(1) != 1 or x.stride(0) % 8 or x.stride(0) < K or x.data_ptr() % 16:
        x = x.contiguous()
    xq = torch.empty(M, K, device=x.device, dtype=torch.float8_e4m3fn)
    sx = torch.empty(M, device=x.device, dtype=torch.float32)
    native().act_quant_fp8(x, xq, sx)
    return xq, sx


def w8a8_gemv(xq: torch.Tensor, sx: torch.Tensor, w, out: Optional[torch.Tensor] = None):
    y = _y(xq.shape[0], w, xq, out, w.dtype)
    native().w8a8_gemv(xq, sx, w.q, w.scale, y)
    return y


def w8a8_decode_gemm(xq: torch.Tensor, sx: torch.Tensor, w, bm: int, bn: int, s: int,
                     form: Optional[int] = None, out: Optional[torch.Tensor] = None):
    """y = (xq @ w.q^T) * sx[:, None] * w.scale[None, :] on the W8A8 decode MFMA kernel with block
    tile (bm, bn), split-K s and MFMA form (``W8A8_FORMS``)."""
    y = _y(xq.shape[0], w, xq, out, w.dtype)
    ws, cnt = _dg_splitk_ws(xq.device, w.shape[0], bm, bn, s)
    native().w8a8_decode_gemm(xq, sx, w.q, w.scale, y, ws, cnt, bm, bn, s,
                              W8A8_FORM if form is None else form)
    return y


def w8a8_gemm(xq: torch.Tensor, sx: torch.Tensor, w, out: Optional[torch.Tensor] = None):
    """The same product on the block-tiled large-M kernel (M > 256)."""
    y = _y(xq.shape[0], w, xq, out, w.dtype)
    native().w8a8_gemm(xq, sx, w.q, w.scale, y)
    return y


def _act_fp8_fallback(xq: torch.Tensor, sx: torch.Tensor, w, w16: torch.Tensor) -> torch.Tensor:
    """The 16-bit path on xq widened (exact) and the dequantised weight ``w16``, rows times sx."""
    y = linear_nt(xq.to(w.dtype), w16)
    return (y.float() * sx[:, None]).to(w.dtype)


def w8a8_fallback(xq: torch.Tensor, sx: torch.Tensor, w) -> torch.Tensor:
    """Fake-quant: every e4m3 value is exact in bf16 / fp16, so the 16-bit path on (xq widened,
    W dequantised) followed by the per-row sx computes the same function to within one extra
    16-bit rounding of W * sw (and of the unscaled product)."""
    return _act_fp8_fallback(xq, sx, w, w8_dequant(w))


def _quant_dtype(x: torch.Tensor, w, word: str) -> None:
    """Raises where the activations are not of the model dtype the weight was quantized from
    (``word``: fp8 / mxfp4, for the message)."""
    if x.dtype != w.dtype:
        raise ValueError(f"{word} weight of a {w.dtype} model applied to {x.dtype} activations")


def _quant_args(x: torch.Tensor, w, word: str) -> Optional[torch.Tensor]:
    """The argument check of the quantized GPU routes: raises on a dtype or shape mismatch; the
    empty result for M == 0, else None."""
    _quant_dtype(x, w, word)
    if x.dim() != 2 or x.shape[1] != w.shape[1]:
        raise ValueError(f"activations {tuple(x.shape)} do not match the weight {tuple(w.shape)}")
    return x.new_empty(0, w.shape[0]) if x.shape[0] == 0 else None


def _linear_w8a8(x: torch.Tensor, w) -> torch.Tensor:
    if not use_native(x):
        from .quant import quantize_fp8_tokens

        xq, sx = quantize_fp8_tokens(x)
        return ((xq.float() @ w.q.float().t()) * sx[:, None] * w.scale[None, :]).to(x.dtype)
    if (empty := _quant_args(x, w, "fp8")) is not None:
        return empty
    M = x.shape[0]
    xq, sx = act_quant_fp8(x)
    if W8:
        if M <= 4 and w.shape[0] % 4 == 0:
            return w8a8_gemv(xq, sx, w)
        p = w8a8_plan(M, w)
        if p is not None:
            return w8a8_decode_gemm(xq, sx, w, *p) if M <= 256 else w8a8_gemm(xq, sx, w)
    return w8a8_fallback(xq, sx, w)


# ---- fp8 activations x MXFP4 weights (ops/quant.py Mxfp4Weight, kernels/w4a8_gemm.hip) ----------
# One function on every route (ops/quant.py): the activation-quant kernel once, then by M: M <= 16
# always the BM = 16 decode kernel ((BN, S) from the plan table where listed, else
# ``w4a8_default_plan``); 17 <= M <= 256 the kernel where the measured plan table
# (configs/kernels/w4a8_gemm_plans.json, written by lumen/bench/w4a8_bench.py) lists the bucket;
# everything else the fallback: w4_dequant into the weight-only path's scratch, xq widened exactly
# to 16 bits, the 16-bit path, the rows multiplied by sx.  LUMEN_W8=0 forces that fallback.
W4A8_BMS = (16, 64, 128, 256)
W4A8_BNS = {16: (64, 128), 64: (64, 128), 128: (64, 128), 256: (64,)}   # compiled variants
_w4a8_plans: Optional[dict] = None


def w4a8_plans() -> dict:
    """{(N, K, BM): (BN, S)} of the W4A8 decode GEMM."""
    global _w4a8_plans
    if _w4a8_plans is None:
        _w4a8_plans = load_plans(_plan_path("LUMEN_W4A8_PLANS", "w4a8_gemm_plans.json"))
    return _w4a8_plans


def w4a8_default_plan(N: int, K: int) -> tuple:
    """(BN, S) of the BM = 16 kernel for a shape the table does not list: 64-column tiles and
    enough split-K for two workgroups on each of the 256 CUs (N = 4096: 64 tiles x 8 slices),
    every slice keeping at least four k128 steps."""
    tiles, kt = -(-N // 64), -(-K // 128)
    return 64, max(1, min(-(-512 // tiles), kt // 4, 16))


def w4a8_plan(M: int, w) -> Optional[tuple]:
    """(BM, BN, S) of the decode kernel for this call, None where the fallback runs."""
    if M > 256 or w.shape[0] % 4:
        return None
    bm = next(b for b in W4A8_BMS if M <= b)
    p = w4a8_plans().get((w.shape[0], w.shape[1], bm))
    if p is None and bm == 16:
        p = w4a8_default_plan(*w.shape)
    return (bm,) + tuple(p) if p is not None else None


def w4a8_decode_gemm(xq: torch.Tensor, sx: torch.Tensor, w, bm: int, bn: int, s: int,
                     out: Optional[torch.Tensor] = None):
    """y = (xq @ wdq^T) * sx[:, None] on the W4A8 decode MFMA kernel with block tile (bm, bn) and
    split-K s."""
    y = _y(xq.shape[0], w, xq, out, w.dtype)
    ws, cnt = _dg_splitk_ws(xq.device, w.shape[0], bm, bn, s)
    native().w4a8_decode_gemm(xq, sx, w.q, w.scale, y, ws, cnt, bm, bn, s)
    return y


def w4_dequant(w, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The 16-bit weight of ``w`` (bit-identical to ``w.dequant()``), by default in the fp8
    modes' persistent scratch of the current (device, stream): valid until the next call there."""
    N, K = w.shape
    if K % 16:
        raise ValueError(f"mxfp4 weights on the GPU need K % 16 == 0, got K = {K}")
    if out is None:
        out = _scratch16(w)
    native().w4_dequant(w.q, w.scale, out)
    return out


def w4a8_fallback(xq: torch.Tensor, sx: torch.Tensor, w) -> torch.Tensor:
    """Every e4m3 value is exact in bf16 / fp16, so the 16-bit path on (xq widened, W
    dequantised) followed by the per-row sx computes the same function to within one extra 16-bit
    rounding of the unscaled product (and, in fp16, of a weight outside its range)."""
    return _act_fp8_fallback(xq, sx, w, w4_dequant(w))


def _linear_w4a8(x: torch.Tensor, w) -> torch.Tensor:
    if not use_native(x):
        from .quant import quantize_fp8_tokens

        xq, sx = quantize_fp8_tokens(x)
        return ((xq.float() @ w.dequant_f32().t()) * sx[:, None]).to(x.dtype)
    if (empty := _quant_args(x, w, "mxfp4")) is not None:
        return empty
    M = x.shape[0]
    xq, sx = act_quant_fp8(x)
    p = w4a8_plan(M, w) if W8 else None
    if p is not None:
        return w4a8_decode_gemm(xq, sx, w, *p)
    return w4a8_fallback(xq, sx, w)


# ---- MXFP4 weight-only (Mxfp4Weight.act is None, kernels/w4a16_gemm.hip) -------------------------
# y = round(sum_k f32(x) f32(w.dequant())) on every route, no activation quantizer.  M <= 4: the
# 4-bit rows-per-lane GEMV, always; 5 <= M <= 256: the W4A16 MFMA kernel where the measured plan
# table (configs/kernels/w4a16_gemm_plans.json, written by lumen/bench/w4a16_bench.py) lists the
# bucket; everything else -- prefill / mixed steps, shapes the kernels refuse -- w4_dequant into
# the persistent 16-bit scratch and the 16-bit path unchanged.  LUMEN_W8=0 forces that fallback.
W4A16_BMS = W8_BMS
W4A16_BNS = {64: (64, 128), 128: (64, 128), 256: (64,)}   # compiled (BM, BN) variants
W4A16_GEMV_CFGS = (41, 42, 81, 82)   # 10 R + GS: compiled (rows per wave group, steps in flight)
_w4a16_plans: Optional[dict] = None


def w4a16_plans() -> dict:
    """{(N, K, BM): (BN, S)} of the W4A16 decode GEMM."""
    global _w4a16_plans
    if _w4a16_plans is None:
        _w4a16_plans = load_plans(_plan_path("LUMEN_W4A16_PLANS", "w4a16_gemm_plans.json"))
    return _w4a16_plans


def w4a16_gemv_ok(x: torch.Tensor, w) -> bool:
    return 0 < x.shape[0] <= 4 and _w8_common_ok(x, w) and w.shape[1] % 16 == 0


def w4a16_plan(x: torch.Tensor, w) -> Optional[tuple]:
    """(BM, BN, S) of the MFMA kernel for this call, None where it does not apply."""
    if not (4 < x.shape[0] <= 256 and _w8_common_ok(x, w) and w.shape[1] % 32 == 0):
        return None
    bm = next(b for b in W4A16_BMS if x.shape[0] <= b)
    p = w4a16_plans().get((w.shape[0], w.shape[1], bm))
    return (bm,) + tuple(p) if p is not None else None


def w4a16_gemv(x: torch.Tensor, w, out: Optional[torch.Tensor] = None, cfg: int = 0):
    """y = x @ w.dequant()^T for 1 <= M <= 4 on the 4-bit GEMV (``cfg``: one of
    ``W4A16_GEMV_CFGS`` instead of the measured default)."""
    y = _y(x.shape[0], w, x, out)
    native().w4a16_gemv(x, w.q, w.scale, y, cfg)
    return y


def w4a16_decode_gemm(x: torch.Tensor, w, bm: int, bn: int, s: int,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x @ w.dequant()^T on the W4A16 MFMA kernel with block tile (bm, bn) and split-K s."""
    y = _y(x.shape[0], w, x, out)
    ws, cnt = _dg_splitk_ws(x.device, w.shape[0], bm, bn, s)
    native().w4a16_decode_gemm(x, w.q, w.scale, y, ws, cnt, bm, bn, s)
    return y


def w4a16_fallback(x: torch.Tensor, w) -> torch.Tensor:
    """The 16-bit path on W dequantised (bit-identical to ``w.dequant()``) into the scratch the
    quantized modes share: the same function up to the library GEMM's accumulation order."""
    return linear_nt(x, w4_dequant(w))


def _linear_w4a16(x: torch.Tensor, w) -> torch.Tensor:
    if not use_native(x):
        return (x.float() @ w.dequant().float().t()).to(x.dtype)
    if (empty := _quant_args(x, w, "mxfp4")) is not None:
        return empty
    if W8 and w4a16_gemv_ok(x, w):
        return w4a16_gemv(x, w)
    p = w4a16_plan(x, w) if W8 else None
    if p is not None:
        return w4a16_decode_gemm(x, w, *p)
    return w4a16_fallback(x, w)


def _linear_w8(x: torch.Tensor, w) -> torch.Tensor:
    if w.act == "fp8":
        return _linear_w8a8(x, w)
    if w.act is not None:
        raise ValueError(f"QuantWeight.act must be None or 'fp8', got {w.act}")
    if not use_native(x):
        return x @ w.dequant().to(x.dtype).t()
    # (dtype only: this route's fallback takes whatever torch.matmul takes, as it always has)
    _quant_dtype(x, w, "fp8")
    # the GEMV at every M <= 4: the fastest of the fp8 routes there.  Known loss against 16-bit
    # weights: at M = 3..4 on the wide projections it is slower than the 16-bit GEMV (M = 4:
    # qkv 29.5 vs 25.5 us, gate|up 48.0 vs 38.7 us, profiles/w8_serve)
    if W8 and w8_gemv_ok(x, w):
        y = torch.empty(x.shape[0], w.shape[0], device=x.device, dtype=x.dtype)
        native().w8_gemv(x, w.q, w.scale, y)
        return y
    p = w8_plan(x, w) if W8 else None
    if p is not None:
        return w8_decode_gemm(x, w, *p)
    return linear_nt(x, w8_dequant(w))


def linear_nt(x: torch.Tensor, w) -> torch.Tensor:
    """x [M, K] @ w[N, K]^T -> [M, N]; ``w`` a 16-bit tensor, an fp8 ``QuantWeight`` (with
    ``act="fp8"``: the product of the per-token quantized x, ops/quant.py) or an ``Mxfp4Weight``
    (``act="fp8"``: with the per-token quantized x; ``act=None``: weight-only)."""
    if isinstance(w, QuantWeight):
        return _linear_w8(x, w)
    if isinstance(w, Mxfp4Weight):
        if w.act is None:
            return _linear_w4a16(x, w)
        if w.act != "fp8":
            raise ValueError(f"Mxfp4Weight.act must be None or 'fp8', got {w.act}")
        return _linear_w4a8(x, w)
    if skinny_ok(x, w):
        y = torch.empty(x.shape[0], w.shape[0], device=x.device, dtype=x.dtype)
        native().skinny_gemm(x, w, y)
        return y
    p = dg_plan(x, w)
    if p is not None:
        return decode_gemm(x, w, *p)
    # prefill / mixed steps (M = 2048-4096 tokens): the whole-wave column split where both
    # parts are tuned, as in training (profiles/r5_serve_split)
    return mm_nt(x, w)


# batch <= 4 decode, opt-in (LUMEN_SWIGLU_GEMV=1): SwiGLU formed inside the rows-per-lane weight
# stream, one launch fewer per layer.  Measured slower both ways: the row-group GEMV form 21.4 vs
# 18.5 us per call, the rows-per-lane form 3.085 vs 2.99-3.01 ms per batch-1 decode step (gpurun
# r5_35) -- every workgroup re-reads and re-activates the whole 2 x 11008 gate|up row
SWIGLU_GEMV = os.environ.get("LUMEN_SWIGLU_GEMV", "0") == "1"


def swiglu_linear_nt(gu: torch.Tensor, w) -> torch.Tensor:
    """(silu(gu[:, :F]) * gu[:, F:]) @ w[N, F]^T, the MLP down projection."""
    from .activation import swiglu

    M, F = gu.shape[0], gu.shape[1] // 2
    if isinstance(w, (QuantWeight, Mxfp4Weight)):
        return linear_nt(swiglu(gu), w)
    if (SWIGLU_GEMV and 0 < M <= 4 and gu.dim() == 2 and gu.shape[1] == 2 * F
            and gu.stride(1) == 1 and gu.stride(0) % 8 == 0 and use_native(gu)
            and w.dim() == 2 and w.shape[1] == F and w.is_contiguous() and gu.dtype == w.dtype
            and gu.dtype in (torch.bfloat16, torch.float16) and w.shape[0] % 4 == 0
            and F % 8 == 0 and skinny_ok(gu[:, :F], w)):
        y = torch.empty(M, w.shape[0], device=gu.device, dtype=gu.dtype)
        native().skinny_swiglu_gemm(gu, w, y)
        return y
    return linear_nt(swiglu(gu), w)


# ---- quantized frozen base for training (--base_quantization, kernels/qbase.hip) ---------------
# The frozen projections are stored once, as a weight-only QuantWeight / Mxfp4Weight, and
# dequantised per use into a 16-bit scratch: "nk" = [N, K] for the forward and the NN backward,
# "kn" = [K, N] = W^T for the TN input-gradient GEMM.  The library GEMMs stay as they are.
#
# The pool is separate from the serving scratch above (that one is sized by w8_reserve and
# captured in decode graphs).  One buffer per (device, stream, dtype, projection name, layout),
# shared by every layer and sized to the largest user: weights that one layer's forward or
# backward touches never alias each other, and consecutive layers reuse a buffer in stream order
# (8 buffers for a Llama layer, ~0.8 GB on Llama-2-7B).  A view is valid until the next
# dequant_into of the same key.
QBASE_LAYOUTS = ("nk", "kn")
_qbase_pool: dict = {}


def qbase_check_shape(N: int, K: int) -> None:
    """The shapes the training dequantisers take (every Llama / OPT preset projection)."""
    if K % 16 or N % 8 or K < 16 or N < 8:
        raise ValueError(f"a quantized base needs projections with K % 16 == 0 and N % 8 == 0, "
                         f"got [N, K] = [{N}, {K}]")


def qbase_scratch_bytes(device=None) -> int:
    """Bytes the training dequant pool holds (on ``device``, or everywhere)."""
    return sum(b.numel() * b.element_size() for k, b in _qbase_pool.items()
               if device is None or k[0] == str(device))


def qbase_release() -> None:
    """Drop the training dequant pool (tests, and between benchmark configurations)."""
    _qbase_pool.clear()


def _qbase_scratch(w, layout: str, name: str) -> torch.Tensor:
    N, K = w.shape
    key = _dg_key(w.device) + (w.dtype, name, layout)
    buf = _qbase_pool.get(key)
    if buf is None or buf.numel() < N * K:
        # the superseded buffer is freed by the caching allocator in stream order
        buf = torch.empty(N * K, dtype=w.dtype, device=w.device)
        _qbase_pool[key] = buf
    return buf[:N * K].view((N, K) if layout == "nk" else (K, N))


def qbase_dequant(w, out: torch.Tensor) -> torch.Tensor:
    """``out[:, :K]`` ([N, K] view, row stride ld >= K, ld % 8 == 0) = ``w.dequant()``, bit for
    bit; columns K..ld are not written."""
    native().qbase_dequant(w.q, w.scale, out, out.stride(0))
    return out


def qbase_dequant_t(w, out: torch.Tensor) -> torch.Tensor:
    """``out`` (contiguous [K, N]) = ``w.dequant().t()``, bit for bit."""
    native().qbase_dequant_t(w.q, w.scale, out)
    return out


def dequant_into(w, layout: str = "nk", name: Optional[str] = None) -> torch.Tensor:
    """The 16-bit weight of the weight-only holder ``w``: ``w.dequant()`` ("nk") or its
    transpose ("kn").  On the GPU a view of the training scratch of (device, stream, dtype,
    ``name``, layout) -- ``name`` is the projection's name, by default ``w.name`` or the shape --
    valid until the next call with the same key; elsewhere a fresh tensor."""
    if layout not in QBASE_LAYOUTS:
        raise ValueError(f"layout must be one of {QBASE_LAYOUTS}, got {layout!r}")
    if not isinstance(w, (QuantWeight, Mxfp4Weight)) or w.act is not None:
        raise ValueError("dequant_into takes a weight-only QuantWeight or Mxfp4Weight")
    if not use_native(w.q):
        d = w.dequant()
        return d if layout == "nk" else d.t().contiguous()
    if w.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"a quantized base on the GPU needs a 16-bit model dtype, got {w.dtype}")
    qbase_check_shape(*w.shape)
    if name is None:
        name = getattr(w, "name", None) or f"{w.shape[0]}x{w.shape[1]}"
    out = _qbase_scratch(w, layout, name)
    return qbase_dequant(w, out) if layout == "nk" else qbase_dequant_t(w, out)
