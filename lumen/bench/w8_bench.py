"""Micro-benchmark of the fp8 weight-only projections (kernels/w8_gemm.hip) at the Llama-2-7B
projection shapes, decode batches 1..256.  Per (shape, M) it times, alternated within one process:

1. ``bf16``      the 16-bit ``linear_nt`` (what serving runs without ``--quantization``);
2. ``w8_*``      every fp8 kernel / plan candidate: the GEMV at M <= 4, each compiled (BM, BN) x
                 split-K candidate of the MFMA kernel from M = 5 on;
3. ``fallback``  ``w8_dequant`` into the scratch + the 16-bit path (``LUMEN_W8=0``).

Device events, a warm-up of every variant, ROUNDS x REPS >= 200 timed launches per variant, the
weights rotated over enough copies that every call streams from HBM.  Bytes are computed from
the shapes.  Writes ``w8_bench.json``, a ``README.md`` table and the plan table derived from it
(``w8_gemm_plans.json``: a (N, K, BM) bucket is listed only where one candidate beat the
fallback at every measured M of the bucket) into ``--out``."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

SHAPES = {"qkv": (12288, 4096), "o": (4096, 4096), "gate_up": (22016, 4096),
          "down": (4096, 11008)}
MS = (1, 2, 4, 8, 16, 32, 64, 128, 192, 256)
SPLITS = (1, 2, 4, 8)
ROUNDS, REPS = 5, 40


def nbytes(M, N, K, wbytes):
    """Bytes the product has to move: weights (+ row scales for fp8), x and y."""
    return N * K * wbytes + (4 * N if wbytes == 1 else 0) + 2 * M * K + 2 * M * N


def time_variants(variants, copies):
    """{name: us per launch}: every variant warmed up, then ROUNDS rounds in which each variant
    runs REPS launches back to back (variants alternated round by round); the median round."""
    import torch

    for fn in variants.values():
        for c in range(copies):
            fn(c)
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(REPS):
                fn(i % copies)
            e1.record()
            e1.synchronize()
            rounds[name].append(e0.elapsed_time(e1) * 1e3 / REPS)
    return {k: round(sorted(v)[len(v) // 2], 2) for k, v in rounds.items()}


def candidates(M, N, K):
    from lumen.ops.gemm import W8_BMS, W8_BNS

    bm = next(b for b in W8_BMS if M <= b)
    out = []
    for bn in W8_BNS[bm]:
        tiles = -(-N // bn)
        for s in SPLITS:
            # at most ~4 blocks per CU, at least 4 k64 steps per slice
            if s > 1 and (tiles * s > 1024 or K // 64 // s < 4):
                continue
            out.append((bm, bn, s))
    return out


def derive_plans(rows):
    """One (BN, S) per (N, K, BM) bucket: the candidate with the least total time over the
    bucket's measured M, listed only if it beat the fallback at every one of them."""
    buckets = {}
    for r in rows:
        if r["M"] <= 4:
            continue
        for name, us in r["us"].items():
            if name.startswith("w8_bm"):
                bm, bn, s = (int(t[2:] if t[0] == "b" else t[1:]) for t in name[3:].split("_"))
                buckets.setdefault((r["N"], r["K"], bm), {}).setdefault((bn, s), []).append(
                    (r["M"], us, r["us"]["fallback"]))
    plans = []
    for (N, K, bm), cands in sorted(buckets.items()):
        (bn, s), pts = min(cands.items(), key=lambda kv: sum(p[1] for p in kv[1]))
        if all(us < fb for _, us, fb in pts):
            plans.append({"N": N, "K": K, "BM": bm, "BN": bn, "S": s,
                          "us": {str(m): us for m, us, _ in pts},
                          "fallback_us": {str(m): fb for m, _, fb in pts}})
    return plans


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__)))), "profiles", "w8_serve"))
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--ms", default=",".join(map(str, MS)))
    a = ap.parse_args()

    import torch

    import lumen.ops.gemm as gm
    from lumen.ops._native import native
    from lumen.ops.quant import quantize_fp8_rows
    from lumen.utils.boxcal import box_record, fixed_work
    from lumen.utils.gemm_tuning import load_tuned_gemms

    if not torch.cuda.is_available() or native() is None:
        raise SystemExit("w8_bench needs a GPU and the native extension")
    load_tuned_gemms()
    dev = torch.device("cuda", 0)
    os.makedirs(a.out, exist_ok=True)
    rows = []
    for name in a.shapes.split(","):
        N, K = SHAPES[name]
        # rotate over enough weight copies that every call streams from HBM (> 256 MB MALL)
        copies = max(2, int(600e6 // (N * K)))
        w16 = [(torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16) for _ in range(copies)]
        w8 = [quantize_fp8_rows(w) for w in w16]
        gm.w8_reserve(dev, N * K)
        for M in (int(m) for m in a.ms.split(",")):
            x = torch.randn(M, K, device=dev).to(torch.bfloat16)
            y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)

            def fallback(c):
                gm.W8 = False
                try:
                    return gm.linear_nt(x, w8[c])
                finally:
                    gm.W8 = True

            variants = {"bf16": lambda c: gm.linear_nt(x, w16[c]), "fallback": fallback}
            if M <= 4:
                variants["w8_gemv"] = lambda c: native().w8_gemv(x, w8[c].q, w8[c].scale, y)
            else:
                for bm, bn, s in candidates(M, N, K):
                    variants[f"w8_bm{bm}_bn{bn}_s{s}"] = (
                        lambda c, bm=bm, bn=bn, s=s: gm.w8_decode_gemm(x, w8[c], bm, bn, s, out=y))
            us = time_variants(variants, copies)
            row = {"shape": name, "N": N, "K": K, "M": M, "us": us,
                   "GBps": {k: round(nbytes(M, N, K, 2 if k == "bf16" else 1) / v / 1e3, 1)
                            for k, v in us.items()},
                   "bytes": {"bf16": nbytes(M, N, K, 2), "fp8": nbytes(M, N, K, 1)}}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del w16, w8
        torch.cuda.empty_cache()
    box = box_record(dev, {"launches_per_variant": ROUNDS * REPS}, fixed_work(dev))
    plans = derive_plans(rows)
    with open(os.path.join(a.out, "w8_bench.json"), "w") as f:
        json.dump({"box": box, "rows": rows}, f, indent=1)
    with open(os.path.join(a.out, "w8_gemm_plans.json"), "w") as f:
        json.dump({"source": "lumen/bench/w8_bench.py (profiles/w8_serve/w8_bench.json)",
                   "plans": plans}, f, indent=1)
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(table(rows, box))
    print(json.dumps({"plans": len(plans), "out": a.out}), flush=True)


def table(rows, box) -> str:
    fw = box.get("fixed_work", {})
    out = ["# fp8 weight-only projections: measured (lumen/bench/w8_bench.py)", "",
           f"Box: {json.dumps(box.get('device'))}; fixed work: GEMM "
           f"{fw.get('gemm', {}).get('pflops')} PFLOP/s, HBM read "
           f"{fw.get('hbm_read', {}).get('tbps')} TB/s.", "",
           "us per call (GB/s from the bytes the shapes need).  `best fp8` is the fastest fp8 "
           "kernel / plan candidate, `fallback` the dequant + 16-bit path.", "",
           "| shape | M | bf16 us (GB/s) | best fp8 us (GB/s) | candidate | fallback us (GB/s) |",
           "|---|---|---|---|---|---|"]
    for r in rows:
        k8 = {k: v for k, v in r["us"].items() if k.startswith("w8_")}
        best = min(k8, key=k8.get)
        out.append(f"| {r['shape']} {r['N']}x{r['K']} | {r['M']} | {r['us']['bf16']} "
                   f"({r['GBps']['bf16']}) | {k8[best]} ({r['GBps'][best]}) | {best} | "
                   f"{r['us']['fallback']} ({r['GBps']['fallback']}) |")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main()
