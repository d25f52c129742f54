"""Quantized frozen base for training on the GPU (``--base_quantization fp8 | mxfp4``): the two
dequantisers of kernels/qbase.hip against the holders' ``dequant()`` bit for bit, with every
output a view inside a NaN-filled buffer whose rest must stay untouched, and short training runs
against a 16-bit model that holds the same dequantised weights."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
KINDS = ["fp8", "mxfp4"]
# a single partial tile, the MX half block (K % 32 == 16), an edge tile in N and in K, and
# small-llama's own gate|up and down shapes
SHAPES = [(8, 16), (8, 48), (72, 96), (2752, 512), (512, 1376)]
# ... and a tile grid that is long in either direction
SHAPES_T = SHAPES + [(4096, 64), (64, 4096)]
GUARD = 256  # sentinel elements before and after the output view (keeps it 16-byte aligned)

_cache = {}


def _weight(kind, N, K, dt):
    """(holder on the GPU, its dequant() computed once on the CPU definition)."""
    from lumen.ops.quant import quantize_fp8_rows, quantize_mxfp4_rows

    key = (kind, N, K, dt)
    if key not in _cache:
        g = torch.Generator().manual_seed(1000 * N + K)
        w = (torch.randn(N, K, generator=g) * 0.02).to(dt)
        q = quantize_fp8_rows(w) if kind == "fp8" else quantize_mxfp4_rows(w)
        q.act = None
        ref = q.dequant()
        q.q, q.scale = q.q.cuda(), q.scale.cuda()
        _cache[key] = (q, ref.cuda())
    return _cache[key]


def _guarded(rows, ld, dt):
    """A NaN-filled buffer and its [rows, ld] middle."""
    buf = torch.full((GUARD + rows * ld + GUARD,), float("nan"), dtype=dt, device="cuda")
    return buf, buf[GUARD:GUARD + rows * ld].view(rows, ld)


def _sentinel_intact(buf, rows, ld, cols):
    mid = buf[GUARD:GUARD + rows * ld].view(rows, ld)
    return (bool(buf[:GUARD].isnan().all()) and bool(buf[GUARD + rows * ld:].isnan().all())
            and bool(mid[:, cols:].isnan().all()))


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("pad", [0, 64])
def test_qbase_dequant_bit_exact(N, K, pad, kind, dt):
    from lumen.ops.gemm import qbase_dequant

    w, ref = _weight(kind, N, K, dt)
    ld = K + pad
    buf, mid = _guarded(N, ld, dt)
    out = qbase_dequant(w, mid[:, :K])
    torch.cuda.synchronize()
    assert out.shape == (N, K) and out.stride() == (ld, 1)
    assert not out.isnan().any()
    assert torch.equal(out, ref)
    # columns K..ld and everything around the view: never written
    assert _sentinel_intact(buf, N, ld, K)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,K", SHAPES_T)
def test_qbase_dequant_t_bit_exact(N, K, kind, dt):
    from lumen.ops.gemm import qbase_dequant_t

    w, ref = _weight(kind, N, K, dt)
    buf, mid = _guarded(K, N, dt)
    out = qbase_dequant_t(w, mid)
    torch.cuda.synchronize()
    assert out.shape == (K, N) and out.is_contiguous()
    assert torch.equal(out, ref.t().contiguous())
    assert _sentinel_intact(buf, K, N, N)


@pytest.mark.parametrize("kind", KINDS)
def test_dequant_into_pool(kind):
    """The op-layer entry: both layouts, one buffer per (projection name, layout) sized to the
    largest user, the serving scratch untouched."""
    from lumen.ops import gemm

    gemm.qbase_release()
    dt = torch.bfloat16
    big, rbig = _weight(kind, 2752, 512, dt)
    small, rsmall = _weight(kind, 72, 96, dt)
    serving = dict(gemm._w8_scratch)
    a = gemm.dequant_into(big, "nk", "p")
    assert torch.equal(a, rbig)
    b = gemm.dequant_into(small, "nk", "p")      # reuses p/nk's buffer
    assert b.data_ptr() == a.data_ptr() and torch.equal(b, rsmall)
    t = gemm.dequant_into(big, "kn", "p")        # another layout: another buffer
    assert torch.equal(t, rbig.t()) and t.is_contiguous() and t.data_ptr() != a.data_ptr()
    o = gemm.dequant_into(small, "nk", "other")  # another name: another buffer
    assert o.data_ptr() not in (a.data_ptr(), t.data_ptr())
    assert gemm.qbase_scratch_bytes() == (2 * 2752 * 512 + 72 * 96) * 2
    assert dict(gemm._w8_scratch) == serving
    with pytest.raises(ValueError, match="layout"):
        gemm.dequant_into(big, "tn")
    gemm.qbase_release()


@pytest.mark.parametrize("kind", KINDS)
def test_qbase_argument_checks(kind):
    """Refusals are ``invalid argument`` errors raised before any launch: the sentinel-filled
    outputs stay untouched."""
    from lumen.ops._native import native
    from lumen.ops.quant import quantize_fp8_rows, quantize_mxfp4_rows

    nat, dt = native(), torch.bfloat16
    quant = quantize_fp8_rows if kind == "fp8" else quantize_mxfp4_rows

    def holder(N, K):
        w = quant((torch.randn(N, K) * 0.02).to(dt))
        return w.q.cuda(), w.scale.cuda()

    def refused(fn, *args):
        with pytest.raises(ValueError, match="invalid argument"):
            fn(*args)

    q, s = holder(16, 64)
    buf, mid = _guarded(64, 64, dt)            # room for either layout
    nk, kn = mid[:16, :64], mid.view(-1)[:64 * 16].view(64, 16)
    # K % 16 != 0 (a [16, 72] weight; MXFP4 pads its storage, fp8 does not)
    q72, s72 = holder(16, 72)
    refused(nat.qbase_dequant, q72, s72, torch.empty(16, 72, dtype=dt, device="cuda"), 72)
    refused(nat.qbase_dequant_t, q72, s72, torch.empty(72, 16, dtype=dt, device="cuda"))
    # N % 8 != 0
    q12, s12 = holder(12, 64)
    refused(nat.qbase_dequant, q12, s12, mid[:12, :64], 64)
    refused(nat.qbase_dequant_t, q12, s12, torch.empty(64, 12, dtype=dt, device="cuda"))
    # misaligned output / codes (2-byte and 1-byte offsets from a 16-byte boundary)
    off = buf[GUARD + 1:GUARD + 1 + 16 * 64]
    refused(nat.qbase_dequant, q, s, off.view(16, 64), 64)
    refused(nat.qbase_dequant_t, q, s, off.view(64, 16))
    qoff = torch.empty(q.numel() + 16, dtype=torch.uint8, device="cuda")[1:1 + q.numel()]
    qoff = qoff.view(q.dtype).view(q.shape).copy_(q)
    refused(nat.qbase_dequant, qoff, s, nk, 64)
    refused(nat.qbase_dequant_t, qoff, s, kn)
    # ld: below K, no multiple of 8, not the view's row stride
    refused(nat.qbase_dequant, q, s, nk, 56)
    refused(nat.qbase_dequant, q, s, buf[GUARD:GUARD + 16 * 68].view(16, 68)[:, :64], 68)
    refused(nat.qbase_dequant, q, s, nk, 128)
    # wrong-device output (the host) and a non-contiguous transposed output
    refused(nat.qbase_dequant, q, s, torch.empty(16, 64, dtype=dt), 64)
    refused(nat.qbase_dequant_t, q, s, torch.empty(64, 16, dtype=dt))
    refused(nat.qbase_dequant_t, q, s, mid[:, :16])
    # an output of another shape, an f32 output
    refused(nat.qbase_dequant, q, s, mid[:8, :64], 64)
    refused(nat.qbase_dequant, q, s, torch.empty(16, 64, device="cuda"), 64)
    torch.cuda.synchronize()
    assert bool(buf.isnan().all())
    # ... and the arguments are otherwise fine
    nat.qbase_dequant(q, s, nk, 64)
    torch.cuda.synchronize()
    assert not nk.isnan().any()


# ---- end to end ---------------------------------------------------------------------------------
def _train(monkeypatch, kind, quantized, stage=0, ckpt=False, bwd_wt="all", dtype="bf16",
           steps=4, accum=2):
    """4 steps x 2 accumulation of small-llama, LoRA r16 with dropout 0.1 (after ``_train`` of
    tests/test_zero3_gpu.py).  ``quantized``: the base stored as ``kind``; else the reference: a
    16-bit model whose decoder projections were overwritten with ``dequant()`` of the same
    quantizer's output, without the LoRA fold (a quantized base does not fold)."""
    import lumen.ops.lora as lora_mod
    from lumen.lora import LoraConfig, adapter_state_dict, apply_lora
    from lumen.models import build_model
    from lumen.models.layers import Linear, quantize_base_model
    from lumen.ops import gemm
    from lumen.parallel.dist import init
    from lumen.train.config import load_ds_config
    from lumen.train.engine import ZeroEngine

    monkeypatch.setenv("LUMEN_BWD_WT", bwd_wt)
    if not quantized:
        monkeypatch.setattr(lora_mod, "FOLD", False)
    gemm.qbase_release()
    torch.manual_seed(0)
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
    m = build_model("small-llama", dtype=dt, device=torch.device("cuda"), seed=3)
    n = quantize_base_model(m, kind)
    assert n == 4 * m.config.num_hidden_layers
    if not quantized:
        from lumen.models.layers import dequantize_base_model

        dequantize_base_model(m)
        assert all(mod.qweight is None and mod.weight.numel() for mod in m.modules()
                   if isinstance(mod, Linear))
    apply_lora(m, LoraConfig(r=16, lora_dropout=0.1))
    m.gradient_checkpointing = ckpt
    m.train()
    env = init()
    ds = load_ds_config({"zero_optimization": {"stage": stage},
                         "scheduler": {"type": "WarmupLR",
                                       "params": {"warmup_min_lr": 0, "warmup_max_lr": "auto",
                                                  "warmup_num_steps": "auto"}}},
                        2, accum, 1, 1e-3, dtype_override=dtype)
    eng = ZeroEngine(m, ds, env)
    g = torch.Generator(device="cpu").manual_seed(5)
    losses = []
    for _ in range(steps * accum):
        ids = torch.randint(3, m.config.vocab_size, (2, 64), generator=g).cuda()
        labels = torch.roll(ids, -1, 1)
        loss = eng.forward({"input_ids": ids, "labels": labels})
        eng.backward(loss)
        eng.step()
        losses.append(float(loss))
    eng.sync_params()
    torch.cuda.synchronize()
    lins = [mod for mod in m.modules() if isinstance(mod, Linear) and mod.qweight is not None]
    info = {"quantized": len(lins), "tn": sum(mod.transpose_bwd for mod in lins),
            "cached_wt": sum(mod._wt is not None or mod._wext is not None for mod in lins),
            "scratch": gemm.qbase_scratch_bytes()}
    return adapter_state_dict(m), losses, info


_refs = {}


def _reference(monkeypatch, kind, ckpt, bwd_wt, dtype):
    """The stage-0 16-bit reference of a case, computed once and shared (stage 0 and stage 2 are
    compared with the same one)."""
    key = (kind, ckpt, bwd_wt, dtype)
    if key not in _refs:
        _refs[key] = _train(monkeypatch, kind, False, 0, ckpt, bwd_wt, dtype)
    return _refs[key]


# one axis at a time around the default case (stage 0, TN backward, no checkpointing, bf16)
CASES = [("fp8", 0, "all", False, "bf16"), ("mxfp4", 0, "all", False, "bf16"),
         ("fp8", 2, "all", False, "bf16"), ("mxfp4", 2, "all", False, "bf16"),
         ("fp8", 0, "none", False, "bf16"), ("mxfp4", 0, "none", False, "bf16"),
         ("fp8", 0, "all", "selective", "bf16"), ("mxfp4", 0, "all", "selective", "bf16"),
         ("fp8", 0, "all", "full", "bf16"), ("mxfp4", 0, "all", "full", "bf16"),
         ("fp8", 0, "all", False, "fp16")]


@pytest.mark.parametrize("kind,stage,bwd_wt,ckpt,dtype", CASES)
def test_quantized_base_training_matches_dequantised_16bit(kind, stage, bwd_wt, ckpt, dtype,
                                                           monkeypatch):
    """Equal math over different weight storage: tests/test_zero3_gpu.py's comparison and its
    tolerances (loss within 2e-2 max(1, |ref|), adapters rtol 2e-3 / atol 2e-5)."""
    ref, ref_losses, rinfo = _reference(monkeypatch, kind, ckpt, bwd_wt, dtype)
    got, losses, info = _train(monkeypatch, kind, True, stage, ckpt, bwd_wt, dtype)
    assert rinfo["quantized"] == 0 and rinfo["scratch"] == 0
    # every decoder projection ran from the quantized storage, through the scratch pool, in the
    # backward layout asked for, and cached nothing
    assert info["quantized"] == 8 and info["cached_wt"] == 0
    assert info["tn"] == (8 if bwd_wt == "all" else 0)
    per_layout = (1024 * 512 + 512 * 512 + 2752 * 512 + 512 * 1376) * 2
    assert info["scratch"] == per_layout * (2 if bwd_wt == "all" else 1)
    for a, b in zip(losses, ref_losses):
        print(f"loss {a:.6f} ref {b:.6f}")
        assert abs(a - b) < 2e-2 * max(1.0, abs(b))
    for k in ref:
        print(k, float((got[k] - ref[k]).abs().max()))
        torch.testing.assert_close(got[k], ref[k], rtol=2e-3, atol=2e-5)
