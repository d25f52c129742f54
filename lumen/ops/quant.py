"""Quantization for serving (``--quantization fp8`` weight-only, ``--quantization ptpc_fp8`` with
per-token fp8 activations, ``--quantization mxfp4`` with MXFP4 weights and the same activations,
``--quantization mxfp4_a16`` with MXFP4 weights and 16-bit activations): the quantizers and the
weight holders.

A projection weight ``w [N, K]`` is stored as OCP e4m3fn (``torch.float8_e4m3fn``, gfx950's fp8)
with one f32 scale per output row; activations, accumulation and outputs keep their types.  The
kernels that consume it are in ``kernels/w8_gemm.hip``, the dispatch in ``ops/gemm.py``.  (The
decode MFMA kernels of all four modes take their tile / k-slice map and their in-launch split-K
reduction from ``kernels/dgemm.h``, the GEMVs their dot product and row sum from
``kernels/gemv.h``.)  The weight quantizer runs once per projection at load time in plain torch:
it is not a hot path.
Under ``ptpc_fp8`` (``QuantWeight.act == "fp8"``) the activations are quantized per token row at
run time: ``quantize_fp8_tokens`` is the definition and the CPU path, kernels/w8a8_gemm.hip's
``act_quant_fp8`` the GPU path."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
# floor of a row's amax: an all-zero row gets a finite scale (and quantizes to zeros)
TINY = 1e-12


@dataclass
class QuantWeight:
    q: torch.Tensor       # [N, K] float8_e4m3fn, contiguous
    scale: torch.Tensor   # [N] float32
    dtype: torch.dtype    # model dtype of the activations and outputs
    # None: weight-only (the activations stay 16-bit).  "fp8": W8A8 (--quantization ptpc_fp8), the
    # activations are quantized per token row at run time (quantize_fp8_tokens)
    act: Optional[str] = None

    @property
    def shape(self):
        return self.q.shape

    @property
    def device(self):
        return self.q.device

    @property
    def nbytes(self) -> int:
        return self.q.numel() * self.q.element_size() + self.scale.numel() * self.scale.element_size()

    def dim(self) -> int:
        return 2

    def dequant(self) -> torch.Tensor:
        """The weight the kernels multiply by, rounded once to ``dtype``."""
        return (self.q.float() * self.scale[:, None]).to(self.dtype)


def quantize_fp8_rows(w: torch.Tensor) -> QuantWeight:
    """Per-output-row symmetric e4m3fn quantization of ``w [N, K]``: scale = max(amax_row, tiny) /
    448, q = clamp(w / scale, +-448) converted to e4m3fn.  torch's conversion to e4m3fn does not
    saturate (500.0 becomes NaN), hence the clamp: f32 rounding of the division can land the row
    maximum a hair above 448."""
    if w.dim() != 2:
        raise ValueError(f"quantize_fp8_rows takes a 2-D weight, got {tuple(w.shape)}")
    wf = w.detach().float()
    scale = wf.abs().amax(dim=1).clamp_(min=TINY) / FP8_MAX
    q = (wf / scale[:, None]).clamp_(-FP8_MAX, FP8_MAX).to(FP8).contiguous()
    return QuantWeight(q, scale.contiguous(), w.dtype)


def quantize_fp8_tokens(x: torch.Tensor):
    """Per-token dynamic e4m3fn quantization of the activations ``x [M, K]`` (W8A8,
    ``--quantization ptpc_fp8``): sx[m] = max(amax_k |x[m, k]|, tiny) / 448 in f32, xq = clamp(x /
    sx, +-448) converted to e4m3fn with round-to-nearest-even.  Returns (xq [M, K] e4m3fn
    contiguous, sx [M] f32).  This is the definition: the CPU path, and what kernels/w8a8_gemm.hip's
    act_quant_fp8 reproduces bit for bit."""
    if x.dim() != 2:
        raise ValueError(f"quantize_fp8_tokens takes 2-D activations, got {tuple(x.shape)}")
    xf = x.detach().float()
    amax = xf.abs().amax(dim=1).clamp_(min=TINY)
    # a true f32 division on every device: torch divides a GPU tensor by a Python scalar by
    # multiplying with its reciprocal, which is not the same number
    sx = amax / torch.full_like(amax, FP8_MAX)
    xq = (xf / sx[:, None]).clamp_(-FP8_MAX, FP8_MAX).to(FP8).contiguous()
    return xq, sx.contiguous()


# ---- MXFP4 weights (--quantization mxfp4, W4A8; --quantization mxfp4_a16, W4A16) -----------------
# OCP MX: blocks of 32 consecutive k share one E8M0 (power-of-two) scale, the elements are e2m1
# (fp4: +-{0, .5, 1, 1.5, 2, 3, 4, 6}).  Round to nearest, no calibration.  The kernels that consume
# it are in kernels/w4a8_gemm.hip: gfx950's scaled MFMA takes the codes and the block scales as they
# are stored here; kernels/w4a16_gemm.hip converts them in registers for 16-bit activations.
# The same definition, applied to every cached K / V head row, is the MXFP4 KV cache
# (--kv-cache-dtype mxfp4: ops/attention.py Mxfp4KV, kernels/paged_attention.hip).
MX_BLOCK = 32
E2M1_MAX = 6.0
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


@dataclass
class Mxfp4Weight:
    q: torch.Tensor       # [N, Kp / 2] uint8, Kp = K rounded up to 32: two e2m1 codes per byte, the
    #                       low nibble holds the even k; padding nibbles are zero
    scale: torch.Tensor   # [N, Kp / 32] uint8: biased E8M0 block exponents, 127 = 2^0
    K: int                # the true inner dimension
    dtype: torch.dtype    # model dtype of the activations and outputs
    # "fp8": W4A8 (--quantization mxfp4), the activations are quantized per token row at run time
    # (quantize_fp8_tokens).  None: weight-only (--quantization mxfp4_a16), the activations stay
    # 16-bit: y = round(sum_k f32(x) f32(dequant())), kernels/w4a16_gemm.hip
    act: Optional[str] = "fp8"

    @property
    def shape(self):
        return torch.Size((self.q.shape[0], self.K))

    @property
    def device(self):
        return self.q.device

    @property
    def nbytes(self) -> int:
        return self.q.numel() + self.scale.numel()

    def dim(self) -> int:
        return 2

    def dequant_f32(self) -> torch.Tensor:
        """wdq [N, K] = f32(code) * 2^e, exact in f32."""
        lut = torch.tensor(_E2M1 + tuple(-v for v in _E2M1), dtype=torch.float32,
                           device=self.q.device)
        codes = torch.stack((self.q & 0xF, self.q >> 4), dim=-1).view(self.q.shape[0], -1)
        e = self.scale.to(torch.int32) - 127
        v = torch.ldexp(lut[codes.long()].view(e.shape[0], e.shape[1], MX_BLOCK), e[:, :, None])
        return v.view(e.shape[0], -1)[:, :self.K]

    def dequant(self) -> torch.Tensor:
        """The weight the kernels multiply by, rounded once to ``dtype`` (the identity in bf16:
        every e2m1 x 2^e is a bf16 number)."""
        return self.dequant_f32().to(self.dtype)


def quantize_mxfp4_rows(w: torch.Tensor) -> Mxfp4Weight:
    """MXFP4 quantization of ``w [N, K]`` over blocks of 32 consecutive k (the last block of a row
    may be partial): e = clamp(floor(log2(amax_block)) - 2, -127, 127) from the f32 exponent field
    (0 for an all-zero block), which puts the block maximum in [4, 8); code = e2m1 of clamp(w *
    2^-e, +-6), round to nearest, ties to the even code.  No per-row scale."""
    if w.dim() != 2:
        raise ValueError(f"quantize_mxfp4_rows takes a 2-D weight, got {tuple(w.shape)}")
    N, K = w.shape
    nb = -(-K // MX_BLOCK)
    wf = torch.zeros(N, nb * MX_BLOCK, dtype=torch.float32, device=w.device)
    wf[:, :K] = w.detach().float()
    wf = wf.view(N, nb, MX_BLOCK)
    amax = wf.abs().amax(dim=-1)
    ex = torch.frexp(amax)[1]                 # amax = m * 2^ex, m in [0.5, 1)
    e = torch.where(amax > 0, (ex - 3).clamp(-127, 127), torch.zeros_like(ex)).to(torch.int32)
    a = torch.ldexp(wf, -e[:, :, None]).abs().clamp_(max=E2M1_MAX)
    # the grid's step is 0.5 below 2, 1 below 4 and 2 above; torch.round is half-to-even, which in
    # each range is the even code
    v = torch.where(a < 2, torch.round(a * 2) / 2, torch.where(a < 4, torch.round(a),
                                                               torch.round(a / 2) * 2))
    code = torch.where(v < 2, v * 2, torch.where(v < 4, v + 2, v / 2 + 4)).to(torch.uint8)
    code = (code | ((wf < 0) & (code != 0)).to(torch.uint8) * 8).view(N, nb * MX_BLOCK)
    q = (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()
    return Mxfp4Weight(q, (e + 127).to(torch.uint8).contiguous(), K, w.dtype)
