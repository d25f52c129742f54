"""Micro-benchmark of the MXFP4 weight-only projections (``--quantization mxfp4_a16``,
kernels/w4a16_gemm.hip) at the Llama-2-7B projection shapes, M = 1 .. 256.  Per (shape, M) it
times, alternated within one process as lumen/bench/w4a8_bench.py does (whose helpers it shares):

1. ``bf16``        the 16-bit ``linear_nt``;
2. ``fp8``         the fp8 weight-only route;
3. ``mxfp4``       the W4A8 route (``linear_nt`` on an ``act="fp8"`` Mxfp4Weight, with its
                   ``act_quant_fp8`` launch);
4. ``gemv*``       M <= 4: the W4A16 GEMV as dispatched (``gemv``) and every compiled (rows per wave
                   group, steps in flight) of it (``gemv_r*_g*``);
5. ``w4a16_*``     M >= 5: every compiled (BM, BN) x split-K candidate of the MFMA kernel for the
                   M's bucket;
6. ``fallback``    the mxfp4_a16 fallback (``w4_dequant`` + the 16-bit path).

Writes ``w4a16_bench.json`` and a ``README.md`` table into ``--out`` and the plan table derived
from the rows into ``--plans`` (a (N, K, bucket) is listed only where one candidate beat the
fallback at every measured M of the bucket)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from lumen.bench.w4a8_bench import MS, candidates, derive_plans  # noqa: E402
from lumen.bench.w8_bench import SHAPES, nbytes  # noqa: E402
from lumen.bench.w8a8_bench import time_variants  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w4a16_serve"))
    ap.add_argument("--plans", default=os.path.join(ROOT, "configs", "kernels",
                                                    "w4a16_gemm_plans.json"))
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--ms", default=",".join(map(str, MS)))
    a = ap.parse_args()

    import torch

    import lumen.ops.gemm as gm
    from lumen.ops._native import native
    from lumen.ops.quant import Mxfp4Weight, quantize_fp8_rows, quantize_mxfp4_rows
    from lumen.utils.boxcal import box_record, fixed_work
    from lumen.utils.gemm_tuning import load_tuned_gemms

    if not torch.cuda.is_available() or native() is None:
        raise SystemExit("w4a16_bench needs a GPU and the native extension")
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
        w4 = [quantize_mxfp4_rows(w) for w in w16]
        wa = [Mxfp4Weight(w.q, w.scale, w.K, w.dtype, act=None) for w in w4]
        gm.w8_reserve(dev, N * K)
        for M in (int(m) for m in a.ms.split(",")):
            x = torch.randn(M, K, device=dev).to(torch.bfloat16)
            y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)

            def fallback(c):
                gm.W8 = False
                try:
                    return gm.linear_nt(x, wa[c])
                finally:
                    gm.W8 = True

            variants = {"bf16": lambda c: gm.linear_nt(x, w16[c]),
                        "fp8": lambda c: gm.linear_nt(x, w8[c]),
                        "mxfp4": lambda c: gm.linear_nt(x, w4[c]), "fallback": fallback}
            if M <= 4:
                variants["gemv"] = lambda c: gm.w4a16_gemv(x, wa[c], out=y)
                for cfg in gm.W4A16_GEMV_CFGS:
                    if cfg == 82 and M > 2:
                        continue   # not compiled
                    variants[f"gemv_r{cfg // 10}_g{cfg % 10}"] = (
                        lambda c, cfg=cfg: gm.w4a16_gemv(x, wa[c], out=y, cfg=cfg))
            else:
                for bm, bn, s in candidates(M, N, K, gm.W4A16_BNS):
                    variants[f"w4a16_bm{bm}_bn{bn}_s{s}"] = (
                        lambda c, bm=bm, bn=bn, s=s: gm.w4a16_decode_gemm(x, wa[c], bm, bn, s,
                                                                          out=y))
            us = time_variants(variants, copies, 40)
            row = {"shape": name, "N": N, "K": K, "M": M, "us": us,
                   "bytes": {"bf16": nbytes(M, N, K, 2), "fp8": nbytes(M, N, K, 1),
                             "mxfp4_a16": wa[0].nbytes + 2 * M * K + 2 * M * N}}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del w16, w8, w4, wa
        torch.cuda.empty_cache()
    box = box_record(dev, {"launches_per_variant": "5 x 40"}, fixed_work(dev))
    plans = derive_plans(rows, "w4a16", gm.W4A16_BMS)
    with open(os.path.join(a.out, "w4a16_bench.json"), "w") as f:
        json.dump({"box": box, "rows": rows, "plans": plans}, f, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.plans)), exist_ok=True)
    with open(a.plans, "w") as f:
        json.dump({"source": "lumen/bench/w4a16_bench.py (profiles/w4a16_serve/w4a16_bench.json)",
                   "plans": plans}, f, indent=1)
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(table(rows, box))
    print(json.dumps({"plans": len(plans), "out": a.out}), flush=True)


def table(rows, box) -> str:
    fw = box.get("fixed_work", {})
    out = ["# MXFP4 weight-only (mxfp4_a16, W4A16) projections: measured "
           "(lumen/bench/w4a16_bench.py)", "",
           f"Box: {json.dumps(box.get('device'))}; fixed work: GEMM "
           f"{fw.get('gemm', {}).get('pflops')} PFLOP/s, HBM read "
           f"{fw.get('hbm_read', {}).get('tbps')} TB/s.", "",
           "us per call.  `bf16` is the 16-bit `linear_nt`, `fp8` the fp8 weight-only route, "
           "`mxfp4` the W4A8 route with its `act_quant_fp8` launch, `best W4A16` the fastest "
           "kernel candidate (M <= 4: the GEMV and its (R, GS) variants, `gemv` being the one "
           "`linear_nt` dispatches; M >= 5: the MFMA kernel's (BM, BN, S); `TB/s`: its code, "
           "scale, x and y bytes over its time), `fallback` the mxfp4_a16 fallback.", "",
           "| shape | M | bf16 | fp8 | mxfp4 | gemv | best W4A16 | candidate | TB/s | fallback |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        k4 = {k: v for k, v in r["us"].items() if k.startswith(("w4a16_", "gemv"))}
        best = min(k4, key=k4.get)
        out.append(f"| {r['shape']} {r['N']}x{r['K']} | {r['M']} | {r['us']['bf16']} | "
                   f"{r['us']['fp8']} | {r['us']['mxfp4']} | {r['us'].get('gemv', '')} | "
                   f"{k4[best]} | {best} | {r['bytes']['mxfp4_a16'] / k4[best] / 1e6:.2f} | "
                   f"{r['us']['fallback']} |")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main()
