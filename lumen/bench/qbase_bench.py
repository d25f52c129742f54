"""Benchmark of the quantized frozen base for training (``--base_quantization``,
kernels/qbase.hip).

(a) ``--kernels``: per Llama-2-7B and 70B projection shape, us per call and effective TB/s (code,
    scale and 16-bit output bytes over the time) of the four dequant variants -- fp8 / MXFP4, row
    major (``nk``) / transposed (``kn``) -- next to what the transposed ones replace: the serving
    dequantiser (``w8_dequant`` / ``w4_dequant``) followed by ``transpose_2d``.  Variants are
    alternated within one process (lumen/bench/w8a8_bench.py ``time_variants``) over enough weight
    copies that every call streams from HBM.
(b) ``--train``: bench.py's training configuration (Llama-2-7B, 8 x 512 tokens, LoRA r16) at ZeRO
    stage 2 with a 16-bit, an fp8 and an MXFP4 base, in ONE call on one box: ms per step, peak HBM,
    and the box calibration.  Step times are compared with the 16-bit run of the same call only.

Writes ``qbase_kernels.json`` / ``qbase_train.json`` into ``--out`` (profiles/qbase_train)."""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from lumen.bench.w8a8_bench import time_variants  # noqa: E402

# [N, K] of the decoder projections (q|k|v, o, gate|up, down)
SHAPES = {
    "7b_qkv": (12288, 4096), "7b_o": (4096, 4096), "7b_gate_up": (22016, 4096),
    "7b_down": (4096, 11008),
    "70b_qkv": (10240, 8192), "70b_o": (8192, 8192), "70b_gate_up": (57344, 8192),
    "70b_down": (8192, 28672),
}


def dequant_bytes(kind: str, N: int, K: int) -> int:
    """Bytes one dequant call has to move: codes and scales in, the 16-bit weight out."""
    q = N * K + 4 * N if kind == "fp8" else N * (-(-K // 32)) * 17
    return q + 2 * N * K


def estimate_traffic_gb(cfg) -> dict:
    """The byte-count estimate of the dequant traffic per forward + backward (no recompute):
    every projection dequantised twice (forward nk, backward kn)."""
    from lumen.parallel.memory_plan import _llama_linears

    out = {}
    for kind in ("fp8", "mxfp4"):
        out[kind] = 2 * cfg.num_hidden_layers * sum(
            dequant_bytes(kind, n, k) for _, n, k in _llama_linears(cfg)) / 1e9
    return out


def run_kernels(a, dev) -> list:
    import torch

    import lumen.ops.gemm as gm
    from lumen.ops.quant import Mxfp4Weight, quantize_fp8_rows, quantize_mxfp4_rows
    from lumen.ops.transpose import transpose_2d

    rows = []
    for name in a.shapes.split(","):
        N, K = SHAPES[name]
        # (> 256 MB of codes across the copies: no call finds its input in the Infinity Cache)
        copies = max(2, int(600e6 // (N * K)))
        w8, w4 = [], []
        for _ in range(copies):
            w = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
            w8.append(quantize_fp8_rows(w))
            m = quantize_mxfp4_rows(w)
            w4.append(Mxfp4Weight(m.q, m.scale, m.K, m.dtype, act=None))
            del w, m
        nk = torch.empty(N, K, dtype=torch.bfloat16, device=dev)
        kn = torch.empty(K, N, dtype=torch.bfloat16, device=dev)
        variants = {
            "fp8_nk": lambda c: gm.qbase_dequant(w8[c], nk),
            "fp8_kn": lambda c: gm.qbase_dequant_t(w8[c], kn),
            "mxfp4_nk": lambda c: gm.qbase_dequant(w4[c], nk),
            "mxfp4_kn": lambda c: gm.qbase_dequant_t(w4[c], kn),
            "fp8_serving_dequant": lambda c: gm.w8_dequant(w8[c], nk),
            "mxfp4_serving_dequant": lambda c: gm.w4_dequant(w4[c], nk),
            "fp8_dequant+transpose_2d": lambda c: transpose_2d(gm.w8_dequant(w8[c], nk), out=kn),
            "mxfp4_dequant+transpose_2d": lambda c: transpose_2d(gm.w4_dequant(w4[c], nk), out=kn),
        }
        us = time_variants(variants, copies, a.reps)
        b8, b4 = dequant_bytes("fp8", N, K), dequant_bytes("mxfp4", N, K)
        row = {"shape": name, "N": N, "K": K, "us": us,
               "bytes": {"fp8": b8, "mxfp4": b4},
               "tbps": {k: round((b8 if k.startswith("fp8") else b4) / v / 1e6, 2)
                        for k, v in us.items() if k.endswith(("_nk", "_kn"))}}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del w8, w4, nk, kn, variants
        gc.collect()
        torch.cuda.empty_cache()
    return rows


def run_train(a, dev) -> list:
    import torch

    import lumen.ops.gemm as gm
    from lumen.lora import LoraConfig, apply_lora
    from lumen.models import build_model, get_config
    from lumen.models.layers import quantize_base_model
    from lumen.parallel.dist import init
    from lumen.train.config import load_ds_config
    from lumen.train.engine import ZeroEngine

    env = init()
    cfg = get_config(a.model)
    rows = []
    for kind in a.kinds.split(","):
        gm.qbase_release()
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)   # nothing of the previous configuration left
        ds = load_ds_config(a.config, a.micro_batch, 1, 1, 2e-4, dtype_override="bf16")
        torch.manual_seed(1234)
        model = build_model(a.model, dtype=ds.torch_dtype, device=dev, init="random", seed=0)
        if kind != "none":
            quantize_base_model(model, kind)
            torch.cuda.empty_cache()
        apply_lora(model, LoraConfig(r=16, lora_dropout=0.05))
        model.gradient_checkpointing = a.gradient_checkpointing
        model.train()
        engine = ZeroEngine(model, ds, env)
        g = torch.Generator(device="cpu").manual_seed(4321)
        batches = []
        for _ in range(4):
            ids = torch.randint(3, cfg.vocab_size, (a.micro_batch, a.seq_len), generator=g)
            labels = torch.full_like(ids, -100)
            labels[:, :-1] = ids[:, 1:]
            batches.append({"input_ids": ids.to(dev), "labels": labels.to(dev),
                            "n_valid": int((labels != -100).sum())})

        def steps(n):
            for s in range(n):
                loss = engine.forward(batches[s % len(batches)])
                engine.backward(loss)
                engine.step()
            return loss

        load_peak = torch.cuda.max_memory_allocated(dev)   # building + quantizing + the engine
        torch.cuda.reset_peak_memory_stats(dev)
        steps(a.warmup)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.rounds):      # the median of a few windows, each ending in a sync
            t0 = time.perf_counter()
            loss = steps(a.steps)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / a.steps * 1e3)
        row = {"base_quantization": kind, "stage": ds.stage,
               "ms_per_step": round(sorted(times)[len(times) // 2], 3),
               "ms_per_step_windows": [round(t, 3) for t in times],
               "tokens_per_step": a.micro_batch * a.seq_len,
               "peak_hbm_gb": round(max(load_peak, torch.cuda.max_memory_allocated(dev)) / 1e9, 3),
               "peak_load_hbm_gb": round(load_peak / 1e9, 3),
               "peak_step_hbm_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 3),
               "allocated_before_gb": round(before / 1e9, 3),
               "allocated_after_gb": round(torch.cuda.memory_allocated(dev) / 1e9, 3),
               "dequant_scratch_gb": round(gm.qbase_scratch_bytes(dev) / 1e9, 3),
               "loss": round(float(loss.detach()), 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        engine.close()
        # (the loss holds the autograd graph's references to the model's weight_fn closures)
        del engine, model, batches, loss, steps
    gm.qbase_release()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qbase_train"))
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--model", default="llama2-7b")
    ap.add_argument("--kinds", default="none,fp8,mxfp4")
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "ds_config_zero2_mi355x.json"))
    ap.add_argument("--micro_batch", type=int, default=8)
    ap.add_argument("--seq_len", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gradient_checkpointing", action="store_true")
    ap.add_argument("--train_json", default="qbase_train.json")
    a = ap.parse_args()

    import torch

    from lumen.models import get_config
    from lumen.ops._native import native
    from lumen.utils.boxcal import box_record, fixed_work
    from lumen.utils.gemm_tuning import load_tuned_gemms

    if not torch.cuda.is_available() or native() is None:
        raise SystemExit("qbase_bench needs a GPU and the native extension")
    if not (a.kernels or a.train):
        a.kernels = a.train = True
    load_tuned_gemms()
    dev = torch.device("cuda", 0)
    os.makedirs(a.out, exist_ok=True)
    if a.kernels:
        rows = run_kernels(a, dev)
        box = box_record(dev, {"launches_per_variant": f"5 x {a.reps}"}, fixed_work(dev))
        with open(os.path.join(a.out, "qbase_kernels.json"), "w") as f:
            json.dump({"box": box, "rows": rows}, f, indent=1)
    if a.train:
        rows = run_train(a, dev)
        box = box_record(dev, {"steps": f"{a.rounds} x {a.steps}", "warmup": a.warmup},
                         fixed_work(dev))
        est = estimate_traffic_gb(get_config(a.model))
        with open(os.path.join(a.out, a.train_json), "w") as f:
            json.dump({"box": box, "rows": rows, "estimated_dequant_traffic_gb": est}, f, indent=1)
    print(json.dumps({"out": a.out}), flush=True)


if __name__ == "__main__":
    main()
