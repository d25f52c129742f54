"""Quantized frozen base for training (``--base_quantization fp8 | mxfp4``) on the CPU path: a
quantized-base model is the 16-bit model that holds ``dequant()`` of the same weights, bit for bit
(both run the same torch ops on the same values); storage, parameter counts, CLI refusals, the
checkpoint record, and a gloo world-2 run."""
import json
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from lumen.lora import (LoraConfig, adapter_state_dict, apply_lora, count_parameters,
                        load_adapter, read_base_quantization, save_adapter)
from lumen.models import build_model
from lumen.models.layers import (Linear, base_quantization_of, dequantize_base_model,
                                 quantize_base_model)
from lumen.ops.gemm import dequant_into
from lumen.ops.quant import Mxfp4Weight, QuantWeight, quantize_fp8_rows, quantize_mxfp4_rows
from lumen.parallel.dist import init
from lumen.train.config import load_ds_config
from lumen.train.trainer import TrainArgs, Trainer, check_base_quantization

KINDS = ["fp8", "mxfp4"]
CPU = torch.device("cpu")


def _pair(kind, lora, K=48, N=40):
    """(quantized-base Linear, plain Linear loaded with its dequant()), same adapter."""
    torch.manual_seed(0)
    w = torch.randn(N, K) * 0.02
    a, b = Linear(K, N, dtype=torch.float32), Linear(K, N, dtype=torch.float32)
    a.weight.data.copy_(w)
    holder = a.quantize_base(kind, "proj")
    b.weight.data.copy_(holder.dequant())
    if lora:
        for m in (a, b):
            m.add_lora(["proj"], 4, 8.0, 0.0)
        with torch.no_grad():
            a.lora.lora_B.normal_(0, 0.05)
            b.lora.lora_A.copy_(a.lora.lora_A)
            b.lora.lora_B.copy_(a.lora.lora_B)
    return a, b, holder


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lora", [False, True])
def test_quantized_linear_equals_dequantised_linear(kind, lora):
    a, b, holder = _pair(kind, lora)
    assert isinstance(holder, QuantWeight if kind == "fp8" else Mxfp4Weight) and holder.act is None
    assert a.weight.numel() == 0 and tuple(a.weight._zero_shape) == (40, 48)
    assert torch.equal(a.weight_fn(), b.weight)
    x = torch.randn(6, 48)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = a(xa), b(xb)
    assert torch.equal(ya, yb)
    g = torch.randn_like(ya)
    ya.backward(g)
    yb.backward(g)
    assert torch.equal(xa.grad, xb.grad)
    if lora:
        assert torch.equal(a.lora.lora_A.grad, b.lora.lora_A.grad)
        assert torch.equal(a.lora.lora_B.grad, b.lora.lora_B.grad)
        assert a.lora.lora_B.grad.abs().sum() > 0


@pytest.mark.parametrize("kind", KINDS)
def test_linear_overrides(kind):
    a, b, holder = _pair(kind, True)
    # the static fold query agrees with the other: a quantized base never folds
    assert a.fold_ext(static=True) == 0 and a.fold_ext() == 0 and a.fold_weight() is None
    # W^T only where the transposed backward is on, and nothing is cached either way
    assert a.weight_t_fn() is None
    a.transpose_bwd = True
    assert torch.equal(a.weight_t_fn(), b.weight.t().contiguous())
    assert a._wt is None and a._wext is None
    a.invalidate_weight_cache()
    assert a.qweight is holder
    with pytest.raises(RuntimeError, match="merge_lora.py"):
        a.merge_lora()
    with pytest.raises(RuntimeError, match="already"):
        a.quantize_base(kind)
    with pytest.raises(ValueError, match="fp8"):
        Linear(16, 8, dtype=torch.float32).quantize_base("nf4")
    # the shapes the GPU dequantisers take are checked once, here
    for K, N in ((40, 8), (48, 12)):
        lin = Linear(K, N, dtype=torch.float32)
        lin.weight.data.normal_()
        with pytest.raises(ValueError, match=r"K % 16 == 0 and N % 8 == 0"):
            lin.quantize_base(kind)
    t = Linear(16, 8, dtype=torch.float32)
    t.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match="frozen"):
        t.quantize_base(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_dequant_into_cpu(kind):
    w = (quantize_fp8_rows if kind == "fp8" else quantize_mxfp4_rows)(torch.randn(24, 48) * 0.02)
    w.act = None
    assert torch.equal(dequant_into(w, "nk"), w.dequant())
    t = dequant_into(w, "kn")
    assert t.is_contiguous() and torch.equal(t, w.dequant().t())
    with pytest.raises(ValueError, match="layout"):
        dequant_into(w, "tn")
    w.act = "fp8"
    with pytest.raises(ValueError, match="weight-only"):
        dequant_into(w, "nk")
    with pytest.raises(ValueError, match="weight-only"):
        dequant_into(torch.zeros(8, 16), "nk")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["tiny-llama", "tiny-opt"])
def test_quantize_base_model(name, kind):
    m = build_model(name, dtype=torch.float32, device=CPU, init="random", seed=1)
    ref = build_model(name, dtype=torch.float32, device=CPU, init="random", seed=1)
    before = count_parameters(m)
    keep = {k: v.clone() for k, v in m.state_dict().items()
            if "embed" in k or "lm_head" in k or "norm" in k}
    n = quantize_base_model(m, kind)
    assert n == 4 * m.config.num_hidden_layers and base_quantization_of(m) == kind
    assert count_parameters(m) == before
    qlins = [(k, mod) for k, mod in m.named_modules()
             if isinstance(mod, Linear) and mod.qweight is not None]
    assert len(qlins) == n and all(k.startswith("layers.") for k, _ in qlins)
    assert all(mod.weight.numel() == 0 for _, mod in qlins)
    # every other linear (the LM head), the embeddings and the norms: untouched
    others = [mod for k, mod in m.named_modules() if isinstance(mod, Linear) and mod.qweight is None]
    assert all(mod.weight.numel() == mod.in_features * mod.out_features for mod in others)
    sd = m.state_dict()
    assert keep and all(torch.equal(sd[k], v) for k, v in keep.items())
    # what the projections keep resident is the holders, nothing else
    persistent = sum(p.numel() * p.element_size() for _, mod in qlins
                     for p in mod.parameters(recurse=False) if p is mod.weight)
    assert persistent == 0
    holders = sum(mod.qweight.nbytes for _, mod in qlins)
    per_elem = 1.0 if kind == "fp8" else 17 / 32
    numel = sum(mod.in_features * mod.out_features for _, mod in qlins)
    assert numel * per_elem <= holders <= numel * per_elem * 1.2
    # the same function as the 16-bit model with dequantised weights
    rmods = dict(ref.named_modules())
    for k, mod in qlins:
        rmods[k].weight.data.copy_(mod.qweight.dequant())
    ids = torch.randint(3, m.config.vocab_size, (2, 12), generator=torch.Generator().manual_seed(2))
    m.eval()
    ref.eval()
    with torch.no_grad():
        assert torch.equal(m(ids), ref(ids))
    # order: before apply_lora
    m2 = build_model(name, dtype=torch.float32, device=CPU, init="random", seed=1)
    apply_lora(m2, LoraConfig(r=4))
    with pytest.raises(RuntimeError, match="before apply_lora"):
        quantize_base_model(m2, kind)
    # and back: 16-bit storage of the same function
    dequantize_base_model(m)
    assert base_quantization_of(m) == "none" and count_parameters(m) == before
    with torch.no_grad():
        assert torch.equal(m(ids), ref(ids))


def _ds(stage=2, **zero):
    return load_ds_config({"zero_optimization": dict(stage=stage, **zero)}, 2, 1, 1, 5e-3,
                          dtype_override="fp32")


def test_cli_flag_parses():
    from lumen.cli.train import VARIANTS, build_parser

    for variant in VARIANTS:
        extra = ["--deepspeed", "x.json"] if variant == "zero3" else []
        p = build_parser(variant)
        assert p.parse_args(extra).base_quantization == "none"
        for kind in KINDS:
            assert p.parse_args(extra + ["--base_quantization", kind]).base_quantization == kind
        with pytest.raises(SystemExit):
            p.parse_args(extra + ["--base_quantization", "nf4"])
    assert TrainArgs().base_quantization == "none"


@pytest.mark.parametrize("kind", KINDS)
def test_refused_configurations(kind, monkeypatch):
    for name in ("LUMEN_FUSED_MLP", "LUMEN_MLP_OVERLAP", "LUMEN_LORA_BWD_OVERLAP"):
        monkeypatch.delenv(name, raising=False)
    check_base_quantization("none", _ds(3))            # the default: nothing is refused
    for stage in (0, 1, 2):
        check_base_quantization(kind, _ds(stage))
    check_base_quantization(kind, _ds(2, offload_optimizer={"device": "cpu"}))
    with pytest.raises(ValueError, match="ZeRO stage 3"):
        check_base_quantization(kind, _ds(3))
    with pytest.raises(ValueError, match="offload_param"):
        check_base_quantization(kind, _ds(2, offload_param={"device": "cpu"}))
    for name in ("LUMEN_FUSED_MLP", "LUMEN_MLP_OVERLAP", "LUMEN_LORA_BWD_OVERLAP"):
        monkeypatch.setenv(name, "1")
        with pytest.raises(ValueError, match=name):
            check_base_quantization(kind, _ds(2))
        monkeypatch.delenv(name)
    with pytest.raises(ValueError, match="none, fp8 or mxfp4"):
        check_base_quantization("nf4", _ds(2))
    # the trainer refuses at startup, before it builds anything ...
    a = TrainArgs(model_name="tiny-llama", synthetic=True, base_quantization=kind)
    with pytest.raises(ValueError, match="ZeRO stage 3"):
        Trainer(a, _ds(3), init(device="cpu"), printer=lambda *x, **k: None)
    # ... and so does the engine for a model quantized by hand
    from lumen.train.engine import ZeroEngine

    m = build_model("tiny-llama", dtype=torch.float32, device=CPU, init="random")
    quantize_base_model(m, kind)
    apply_lora(m, LoraConfig(r=4))
    with pytest.raises(ValueError, match="ZeRO stage 3"):
        ZeroEngine(m, _ds(3), init(device="cpu"))


def _trainer(out, kind, max_steps, resume=False):
    a = TrainArgs(model_name="tiny-llama", synthetic=True, synthetic_samples=40, max_length=16,
                  per_device_train_batch_size=2, gradient_accumulation_steps=1,
                  max_steps=max_steps, logging_steps=1, lora_r=4, lora_dropout=0.0,
                  save_strategy="steps", save_steps=2, resume_from_checkpoint=resume,
                  output_dir=out, seed=3, save_final=True, async_save=False,
                  base_quantization=kind)
    return Trainer(a, _ds(1), init(device="cpu"), printer=lambda *x, **k: None)


def test_checkpoint_records_base_quantization(tmp_path):
    out = str(tmp_path / "run")
    t = _trainer(out, "fp8", 2)
    assert t.n_total == count_parameters(build_model("tiny-llama", dtype=torch.float32,
                                                     device=CPU))[1] + t.n_trainable
    t.train()
    ck = os.path.join(out, "checkpoint-2")
    with open(os.path.join(ck, "trainer_state.json")) as f:
        st = json.load(f)
    assert st["base_quantization"] == "fp8" and st["args"]["base_quantization"] == "fp8"
    for d in (ck, os.path.join(out, "final")):
        with open(os.path.join(d, "adapter_config.json")) as f:
            assert json.load(f)["lumen_base_quantization"] == "fp8"
        assert read_base_quantization(d) == "fp8"
    # PEFT-format loading is unaffected by the extra key
    m = build_model("tiny-llama", dtype=torch.float32, device=CPU, init="random", seed=3)
    load_adapter(m, os.path.join(out, "final"))
    want = adapter_state_dict(t.model)
    got = adapter_state_dict(m)
    assert want.keys() == got.keys() and all(torch.equal(want[k], got[k]) for k in want)
    # resuming under another storage of the base is refused, under the same one it runs on
    for other in ("none", "mxfp4"):
        with pytest.raises(ValueError, match="--base_quantization fp8"):
            _trainer(out, other, 4, resume=True).train()
    again = _trainer(out, "fp8", 4, resume=True)
    again.train()
    assert again.engine.global_step == 4
    # a 16-bit run records "none", and an adapter directory without the key reads as "none"
    m16 = build_model("tiny-llama", dtype=torch.float32, device=CPU, init="random")
    apply_lora(m16, LoraConfig(r=4))
    save_adapter(m16, str(tmp_path / "a16"))
    assert read_base_quantization(str(tmp_path / "a16")) == "none"
    with open(tmp_path / "a16" / "adapter_config.json") as f:
        conf = json.load(f)
    del conf["lumen_base_quantization"]
    with open(tmp_path / "a16" / "adapter_config.json", "w") as f:
        json.dump(conf, f)
    assert read_base_quantization(str(tmp_path / "a16")) == "none"


def test_memory_plan_counts_quantized_bytes_and_scratch():
    from lumen.models import get_config
    from lumen.parallel.memory_plan import plan_replicated, qbase_bytes, qbase_scratch_bytes

    cfg = get_config("llama2-7b")
    lin = 32 * (3 * 4096 * 4096 + 4096 * 4096 + 3 * 4096 * 11008)
    assert qbase_bytes(cfg, "none") == 2 * lin
    assert lin < qbase_bytes(cfg, "fp8") < 1.001 * lin
    assert qbase_bytes(cfg, "mxfp4") == lin * 17 / 32
    assert qbase_scratch_bytes(cfg, True) == 2 * 2 * lin / 32
    assert qbase_scratch_bytes(cfg, False) == 2 * lin / 32
    p16, p8, p4 = (plan_replicated(cfg, 288e9, 4096, k, "none") for k in ("none", "fp8", "mxfp4"))
    # 16-bit: W and W^T; quantized: the holders once plus the 8-buffer scratch (~0.8 GB)
    assert p16["gb"]["w_transposed"] == p16["gb"]["projections"] and p16["gb"]["dequant_scratch"] == 0
    for p in (p8, p4):
        assert p["gb"]["w_transposed"] == 0 and 0.7 < p["gb"]["dequant_scratch"] < 0.9
    # ... and no LoRA fold copies ([N, K + 64] of the adapted q|k|v and o)
    fold = 32 * 2 * (3 * 4096 + 4096) * (4096 + 64)
    assert abs(p16["gb"]["lora_fold"] - fold / 1e9) < 1e-9 and p8["gb"]["lora_fold"] == 0
    saved8 = p16["peak_gb"] - p8["peak_gb"]
    assert abs(saved8 - (4 * lin + fold - qbase_bytes(cfg, "fp8") - qbase_scratch_bytes(cfg))
               / 1e9) < 1e-6
    # within 10 % of the measured resident bytes (profiles/qbase_train: 31.8 / 8.9 / 5.9 GB)
    for p, measured in ((p16, 31.80), (p8, 8.91), (p4, 5.90)):
        g = p["gb"]
        resident = (g["projections"] + g["embed_head"] + g["lora_state"] + g["w_transposed"]
                    + g["lora_fold"] + g["dequant_scratch"])
        assert abs(resident - measured) < 0.1 * measured, (resident, measured)
    assert p4["peak_gb"] < p8["peak_gb"] < p16["peak_gb"]


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, stage, outdir, kind, micro, steps=3):
    from tests._qbase_worker import train_worker

    os.makedirs(outdir, exist_ok=True)
    port = _port()
    if world == 1:
        train_worker(0, 1, port, stage, outdir, kind, micro, steps)
    else:
        mp.spawn(train_worker, args=(world, port, stage, outdir, kind, micro, steps),
                 nprocs=world, join=True)
    return torch.load(os.path.join(outdir, f"result_stage{stage}_w{world}.pt"), weights_only=True)


def test_zero2_world2_fp8_matches_single_process(tmp_path):
    """tests/test_zero_gloo.py's comparison (same global batch: world 2 x micro 2 vs world 1 x
    micro 4) and its tolerances, over an fp8 base."""
    ref = _run(1, 0, str(tmp_path / "ref"), "fp8", 4)
    r = _run(2, 2, str(tmp_path / "w2"), "fp8", 2)
    assert ref["quantized"] == r["quantized"] == 8
    assert len(r["losses"]) == len(ref["losses"]) == 3
    for a, b in zip(r["losses"], ref["losses"]):
        assert abs(a - b) < 1e-3
    assert r["sd"].keys() == ref["sd"].keys()
    for k in ref["sd"]:
        assert torch.allclose(r["sd"][k], ref["sd"][k], atol=2e-5, rtol=1e-4), k
    assert any(v.abs().sum() > 0 for k, v in r["sd"].items() if "lora_B" in k)


def test_evaluate_over_the_base_the_adapter_saw(tmp_path, capsys):
    """scripts/evaluate.py --base_quantization: the loss pass runs over the quantized base, the
    generation pass merges into its 16-bit dequantised form, and a mismatch with the adapter's
    recorded value is reported."""
    import importlib.util

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("lumen_evaluate",
                                                  os.path.join(root, "scripts", "evaluate.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    m = build_model("tiny-llama", dtype=torch.float32, device=CPU)
    quantize_base_model(m, "fp8")
    apply_lora(m, LoraConfig(r=4))
    with torch.no_grad():
        for p in m.parameters():
            if p.requires_grad:
                p.normal_(0, 0.02)
    ad = str(tmp_path / "adapter")
    save_adapter(m, ad)
    common = ["--model", "tiny-llama", "--adapter", ad, "--synthetic", "--max_samples", "4",
              "--max_length", "32"]
    q = ev.main(common + ["--gen_samples", "2", "--max_new_tokens", "4",
                          "--base_quantization", "fp8"])
    assert q["base_quantization"] == "fp8" and q["generation"]["n"] == 2
    assert "warning" not in capsys.readouterr().err
    plain = ev.main(common + ["--skip_generation"])
    assert "trained with --base_quantization fp8" in capsys.readouterr().err
    # another base function: close, not equal
    assert plain["eval_loss"] != q["eval_loss"] and abs(plain["eval_loss"] - q["eval_loss"]) < 0.05
