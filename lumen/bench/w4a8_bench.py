"""Micro-benchmark of the MXFP4-weight projections (``--quantization mxfp4``,
kernels/w4a8_gemm.hip) at the Llama-2-7B projection shapes, M = 1 .. 256.  Per (shape, M) it times,
alternated within one process as lumen/bench/w8a8_bench.py does:

1. ``bf16``       the 16-bit ``linear_nt``;
2. ``fp8``        the weight-only route (``linear_nt`` on an ``act=None`` QuantWeight);
3. ``ptpc_fp8``   the W8A8 route (``linear_nt`` on an ``act="fp8"`` QuantWeight);
4. ``w4a8_*``     every compiled (BM, BN) x split-K candidate of the decode kernel for the M's
                  bucket WITH its ``act_quant_fp8`` launch;
5. ``fallback``   the mxfp4 fallback (activation quantizer, ``w4_dequant``, the 16-bit path, the
                  row scales).

Writes ``w4a8_bench.json``, a ``README.md`` table and the plan table derived from it
(``w4a8_gemm_plans.json``: a (N, K, bucket) is listed only where one candidate beat the fallback at
every measured M of the bucket) into ``--out``."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from lumen.bench.w8_bench import SHAPES, nbytes  # noqa: E402
from lumen.bench.w8a8_bench import time_variants  # noqa: E402

MS = (1, 2, 4, 8, 16, 32, 64, 128, 192, 256)
SPLITS = (1, 2, 4, 8, 16)


def bucket_of(M, bms=None):
    """The block height that serves M rows (``bms``: another kernel's block heights)."""
    if bms is None:
        from lumen.ops.gemm import W4A8_BMS as bms

    return next(b for b in bms if M <= b)


def candidates(M, N, K, bns=None):
    """Every (BM, BN, S) to time at M rows (``bns``: another kernel's compiled variants)."""
    if bns is None:
        from lumen.ops.gemm import W4A8_BNS as bns

    bm = bucket_of(M, sorted(bns))
    out = []
    for bn in bns[bm]:
        tiles = -(-N // bn)
        for s in SPLITS:
            # at most ~4 blocks per CU, at least 4 k128 steps per slice
            if s > 1 and (tiles * s > 1024 or -(-K // 128) // s < 4):
                continue
            out.append((bm, bn, s))
    return out


def derive_plans(rows, prefix="w4a8", bms=None):
    """One (BN, S) per (N, K, bucket): the ``prefix``_bm*_bn*_s* candidate with the least total
    time over the bucket's measured M, listed only if it beat the fallback at every one of them."""
    buckets = {}
    for r in rows:
        for name, us in r["us"].items():
            if not name.startswith(prefix + "_bm"):
                continue
            _, bn, s = (int(t.lstrip("bmns")) for t in name[len(prefix) + 1:].split("_"))
            buckets.setdefault((r["N"], r["K"], bucket_of(r["M"], bms)), {}).setdefault(
                (bn, s), []).append((r["M"], us, r["us"]["fallback"]))
    plans = []
    for (N, K, b), cands in sorted(buckets.items()):
        (bn, s), pts = min(cands.items(), key=lambda kv: sum(p[1] for p in kv[1]))
        if all(us < fb for _, us, fb in pts):
            plans.append({"N": N, "K": K, "BM": b, "BN": bn, "S": s,
                          "us": {str(m): us for m, us, _ in pts},
                          "fallback_us": {str(m): fb for m, _, fb in pts}})
    return plans


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__)))), "profiles", "w4a8_serve"))
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--ms", default=",".join(map(str, MS)))
    a = ap.parse_args()

    import torch

    import lumen.ops.gemm as gm
    from lumen.ops._native import native
    from lumen.ops.quant import QuantWeight, quantize_fp8_rows, quantize_mxfp4_rows
    from lumen.utils.boxcal import box_record, fixed_work
    from lumen.utils.gemm_tuning import load_tuned_gemms

    if not torch.cuda.is_available() or native() is None:
        raise SystemExit("w4a8_bench needs a GPU and the native extension")
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
        wa = [QuantWeight(w.q, w.scale, w.dtype, act="fp8") for w in w8]
        w4 = [quantize_mxfp4_rows(w) for w in w16]
        gm.w8_reserve(dev, N * K)
        for M in (int(m) for m in a.ms.split(",")):
            x = torch.randn(M, K, device=dev).to(torch.bfloat16)
            y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)

            def fallback(c):
                gm.W8 = False
                try:
                    return gm.linear_nt(x, w4[c])
                finally:
                    gm.W8 = True

            variants = {"bf16": lambda c: gm.linear_nt(x, w16[c]),
                        "fp8": lambda c: gm.linear_nt(x, w8[c]),
                        "ptpc_fp8": lambda c: gm.linear_nt(x, wa[c]), "fallback": fallback}
            for bm, bn, s in candidates(M, N, K):
                variants[f"w4a8_bm{bm}_bn{bn}_s{s}"] = (
                    lambda c, bm=bm, bn=bn, s=s: gm.w4a8_decode_gemm(
                        *gm.act_quant_fp8(x), w4[c], bm, bn, s, out=y))
            us = time_variants(variants, copies, 40)
            row = {"shape": name, "N": N, "K": K, "M": M, "us": us,
                   "bytes": {"bf16": nbytes(M, N, K, 2), "fp8": nbytes(M, N, K, 1),
                             "mxfp4": w4[0].nbytes + M * K + 2 * M * N}}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del w16, w8, wa, w4
        torch.cuda.empty_cache()
    box = box_record(dev, {"launches_per_variant": "5 x 40"}, fixed_work(dev))
    plans = derive_plans(rows)
    with open(os.path.join(a.out, "w4a8_bench.json"), "w") as f:
        json.dump({"box": box, "rows": rows, "plans": plans}, f, indent=1)
    with open(os.path.join(a.out, "w4a8_gemm_plans.json"), "w") as f:
        json.dump({"source": "lumen/bench/w4a8_bench.py (profiles/w4a8_serve/w4a8_bench.json)",
                   "plans": plans}, f, indent=1)
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(table(rows, box))
    print(json.dumps({"plans": len(plans), "out": a.out}), flush=True)


def table(rows, box) -> str:
    fw = box.get("fixed_work", {})
    out = ["# MXFP4-weight (mxfp4, W4A8) projections: measured (lumen/bench/w4a8_bench.py)", "",
           f"Box: {json.dumps(box.get('device'))}; fixed work: GEMM "
           f"{fw.get('gemm', {}).get('pflops')} PFLOP/s, HBM read "
           f"{fw.get('hbm_read', {}).get('tbps')} TB/s.", "",
           "us per call.  `bf16` is the 16-bit `linear_nt`, `fp8` the weight-only route, "
           "`ptpc_fp8` the W8A8 route, `best W4A8` the fastest mxfp4 kernel candidate (`TB/s`: its "
           "code, scale, x and y bytes over its time), `fallback` the mxfp4 fallback.  The "
           "ptpc_fp8, W4A8 and fallback times include the `act_quant_fp8` launch.", "",
           "| shape | M | bf16 | fp8 | ptpc_fp8 | best W4A8 | candidate | TB/s | fallback |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        k4 = {k: v for k, v in r["us"].items() if k.startswith("w4a8_")}
        best = min(k4, key=k4.get)
        out.append(f"| {r['shape']} {r['N']}x{r['K']} | {r['M']} | {r['us']['bf16']} | "
                   f"{r['us']['fp8']} | {r['us']['ptpc_fp8']} | {k4[best]} | {best} | "
                   f"{r['bytes']['mxfp4'] / k4[best] / 1e6:.2f} | {r['us']['fallback']} |")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main()
