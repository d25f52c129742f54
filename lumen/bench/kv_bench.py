"""Benchmark of the KV-cache types (``--kv-cache-dtype auto | fp8 | mxfp4``): one call on one box
writes ``kv_bench.json`` and a ``README.md`` into ``--out`` (profiles/kv_mxfp4).

1. Paged decode, one layer, per cache type (alternated round by round within the process): Llama-2
   7B heads (32 / 32, D = 128) and the 70B GQA heads (64 / 8) at 256 sequences x 576 tokens,
   32 x 4096 and 1 x 4096; us per call and effective TB/s (the K + V bytes of the cached tokens in
   that type over the time).  Calls rotate over enough disjoint sets of cache blocks that every
   call streams from HBM (more than the 256 MB the chip can keep on die).
2. The cache write and the fused RoPE + write at T = 256 and T = 4096 (7B heads), us per call.
3. ``serve_bench`` engine mode (Llama-2-7B preset, random init), 512 in / 128 out, 1 and 256
   requests, one fresh process per cache type: ITL p50 / p99, output tok/s, TTFT p50, KV blocks.

Every comparison in the table is between runs of this one call."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

KINDS = ("bf16", "fp8", "mxfp4")
HEADS = {"llama2-7b": (32, 32), "llama2-70b-gqa": (64, 8)}
LOADS = ((256, 576), (32, 4096), (1, 4096))
D, BS = 128, 16
ROW_BYTES = {"bf16": 2 * D, "fp8": D, "mxfp4": D // 2 + D // 32}


def make_cache(kind, nblocks, nkv, dev):
    """A K and a V cache of ``kind`` holding valid random values (never read for their meaning)."""
    import torch

    from lumen.ops.attention import Mxfp4KV

    out = []
    for _ in range(2):
        if kind == "mxfp4":
            c = Mxfp4KV(nblocks, nkv, BS, D, dev)
            c.codes.copy_(torch.randint(0, 256, c.codes.shape, device=dev, dtype=torch.uint8))
            c.scale.copy_(torch.randint(122, 130, c.scale.shape, device=dev, dtype=torch.uint8))
        else:
            c = torch.empty(nblocks, nkv, BS, D, device=dev, dtype=torch.bfloat16).normal_()
            if kind == "fp8":
                c = c.to(torch.float8_e4m3fn)
        out.append(c)
    return out


def bench_decode(dev):
    import torch

    from lumen.bench.w8a8_bench import time_variants
    from lumen.ops.attention import paged_decode

    rows = []
    for name, (nh, nkv) in HEADS.items():
        for nseq, ctx in LOADS:
            maxb = -(-ctx // BS)
            live = {k: 2 * nseq * ctx * nkv * ROW_BYTES[k] for k in KINDS}
            copies = min(40, max(2, math.ceil(600e6 / live["mxfp4"])))
            nblocks = copies * nseq * maxb
            tables = torch.randperm(nblocks, device=dev).int().view(copies, nseq, maxb)
            cl = torch.full((nseq,), ctx, dtype=torch.int32, device=dev)
            q = torch.randn(nseq, nh, D, device=dev).to(torch.bfloat16)
            # the engine's partition rule (ModelRunner.decode_partition, LUMEN_PA_PARTITION 2048)
            part = 2048
            while part > 64 and nseq * nkv * (2048 // part) < 2048:
                part //= 2
            us = {}
            for kind in KINDS:   # one type resident at a time: 16-bit 256 x 576 x 2 sets is 4.8 GB
                kc, vc = make_cache(kind, nblocks, nkv, dev)
                fn = lambda c, kc=kc, vc=vc: paged_decode(q, kc, vc, tables[c], cl, ctx,  # noqa: E731
                                                          1 / math.sqrt(D), part)
                us.update(time_variants({kind: fn}, copies, 20))
                del kc, vc, fn
                torch.cuda.empty_cache()
            row = {"heads": name, "nh": nh, "nkv": nkv, "seqs": nseq, "ctx": ctx,
                   "partition": part, "block_sets": copies, "us": us, "kv_bytes": live,
                   "tbps": {k: round(live[k] / us[k] / 1e6, 2) for k in KINDS}}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def bench_write(dev):
    import torch

    from lumen.bench.w8a8_bench import time_variants
    from lumen.ops.attention import rope_write_kv, write_kv_cache
    from lumen.ops.rope import rope_tables

    nh, nkv = HEADS["llama2-7b"]
    cos, sin = rope_tables(D, 4096, 10000.0, dev)
    rows = []
    for T in (256, 4096):
        nblocks = 2 * T // BS
        qkv = torch.randn(T, (nh + 2 * nkv) * D, device=dev).to(torch.bfloat16)
        k = qkv[:, nh * D:(nh + nkv) * D].view(T, nkv, D)
        v = qkv[:, (nh + nkv) * D:].view(T, nkv, D)
        pos = torch.arange(T, device=dev, dtype=torch.int32)
        slots = torch.randperm(nblocks * BS, device=dev)[:T]
        caches = {kind: make_cache(kind, nblocks, nkv, dev) for kind in KINDS}
        wr = {kind: (lambda c, kc=kc, vc=vc: write_kv_cache(k, v, kc, vc, slots))
              for kind, (kc, vc) in caches.items()}
        scr = qkv.clone()
        rp = {kind: (lambda c, kc=kc, vc=vc: rope_write_kv(scr, pos, nh, nkv, D, cos, sin, kc, vc,
                                                            slots))
              for kind, (kc, vc) in caches.items()}
        row = {"T": T, "write_us": time_variants(wr, 1, 40), "rope_write_us": time_variants(rp, 1, 40)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def serve_child(kv, model):
    """One engine of cache type ``kv``: serve_bench engine mode at 1 and 256 requests."""
    from lumen.bench.serve_bench import bench_engine, make_engine

    a = argparse.Namespace(model=model, max_model_len=4096, max_num_seqs=256,
                           max_batched_tokens=2048, prefill_boost=1, no_graphs=False,
                           sync_scheduling=False, kv_cache_dtype=kv, prompt_len=512,
                           max_tokens=128, temperature=0.0, request_rate=None, num_requests=1)
    eng = make_engine(a)
    for n in (1, 256):
        a.num_requests = n
        r = bench_engine(a, eng)
        keep = ("requests", "itl_p50_ms", "itl_p99_ms", "output_tok_s", "ttft_p50_ms",
                "kv_blocks", "preemptions", "wall_s", "hbm")
        print("KVBENCH " + json.dumps({"kv": kv, **{k: r[k] for k in keep}}), flush=True)


def bench_serve(model):
    rows = []
    for kv in ("auto", "fp8", "mxfp4"):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--serve-child", kv,
                            "--model", model], capture_output=True, text=True, cwd=ROOT)
        got = [json.loads(ln[8:]) for ln in p.stdout.splitlines() if ln.startswith("KVBENCH ")]
        if p.returncode != 0 or len(got) != 2:
            raise SystemExit(f"serve run {kv} failed ({p.returncode}):\n{p.stdout[-2000:]}\n"
                             f"{p.stderr[-4000:]}")
        rows += got
        for g in got:
            print(json.dumps(g), flush=True)
    return rows


def table(res) -> str:
    box = res["box"]
    fw = box.get("fixed_work", {})
    out = ["# KV-cache types: 16-bit, fp8 and MXFP4, measured (lumen/bench/kv_bench.py)", "",
           f"Box: {json.dumps(box.get('device'))}; fixed work: GEMM "
           f"{fw.get('gemm', {}).get('pflops')} PFLOP/s, HBM read "
           f"{fw.get('hbm_read', {}).get('tbps')} TB/s.  Every row compares runs of one call.", "",
           "## Paged decode, one layer (D = 128, block size 16)", "",
           "us per call; TB/s = the K + V bytes of the cached tokens in that type over the time. "
           "`mxfp4 / fp8` below 1 means the 4-bit cache is faster.", "",
           "| heads | seqs x ctx | partition | bf16 us | fp8 us | mxfp4 us | bf16 TB/s | fp8 TB/s | "
           "mxfp4 TB/s | mxfp4 / fp8 | mxfp4 / bf16 |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["decode"]:
        u, t = r["us"], r["tbps"]
        out.append(f"| {r['heads']} {r['nh']}/{r['nkv']} | {r['seqs']} x {r['ctx']} | "
                   f"{r['partition']} | {u['bf16']} | {u['fp8']} | {u['mxfp4']} | {t['bf16']} | "
                   f"{t['fp8']} | {t['mxfp4']} | {u['mxfp4'] / u['fp8']:.2f} | "
                   f"{u['mxfp4'] / u['bf16']:.2f} |")
    out += ["", "## Cache write and fused RoPE + write (7B heads, us per call)", "",
            "| T | write bf16 | write fp8 | write mxfp4 | rope+write bf16 | rope+write fp8 | "
            "rope+write mxfp4 |", "|---|---|---|---|---|---|---|"]
    for r in res["write"]:
        w, p = r["write_us"], r["rope_write_us"]
        out.append(f"| {r['T']} | {w['bf16']} | {w['fp8']} | {w['mxfp4']} | {p['bf16']} | "
                   f"{p['fp8']} | {p['mxfp4']} |")
    if res.get("serve"):
        out += ["", f"## serve_bench engine mode ({res['model']}, random init, 512 in / 128 out)", "",
                "| kv cache | requests | ITL p50 ms | ITL p99 ms | output tok/s | TTFT p50 ms | "
                "KV blocks | KV cache GiB |", "|---|---|---|---|---|---|---|---|"]
        for r in res["serve"]:
            out.append(f"| {r['kv']} | {r['requests']} | {r['itl_p50_ms']} | {r['itl_p99_ms']} | "
                       f"{r['output_tok_s']} | {r['ttft_p50_ms']} | {r['kv_blocks']} | "
                       f"{(r.get('hbm') or {}).get('kv_cache_gib')} |")
    else:
        out += ["", "The serve_bench engine runs were not measured in this call (`--skip-serve`)."]
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_mxfp4"))
    ap.add_argument("--model", default="llama2-7b")
    ap.add_argument("--skip-serve", action="store_true")
    ap.add_argument("--serve-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()

    import torch

    from lumen.ops._native import native

    if not torch.cuda.is_available() or native() is None:
        raise SystemExit("kv_bench needs a GPU and the native extension")
    if a.serve_child:
        serve_child(a.serve_child, a.model)
        return
    from lumen.utils.boxcal import box_record, fixed_work

    dev = torch.device("cuda", 0)
    os.makedirs(a.out, exist_ok=True)
    res = {"model": a.model, "decode": bench_decode(dev), "write": bench_write(dev)}
    res["box"] = box_record(dev, {"launches_per_variant": "5 x 20 (decode), 5 x 40 (writes)"},
                            fixed_work(dev))
    torch.cuda.empty_cache()
    res["serve"] = None if a.skip_serve else bench_serve(a.model)
    with open(os.path.join(a.out, "kv_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(table(res))
    print(json.dumps({"out": a.out}), flush=True)


if __name__ == "__main__":
    main()
