"""fp8 quantization for serving (``--quantization fp8`` weight-only, ``--quantization ptpc_fp8``
with per-token fp8 activations): the quantizers and the weight holder.

A projection weight ``w [N, K]`` is stored as OCP e4m3fn (``torch.float8_e4m3fn``, gfx950's fp8)
with one f32 scale per output row; activations, accumulation and outputs keep their types.  The
kernels that consume it are in ``kernels/w8_gemm.hip``, the dispatch in ``ops/gemm.py``.  The
weight quantizer runs once per projection at load time in plain torch: it is not a hot path.
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
