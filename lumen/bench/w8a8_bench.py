"""Micro-benchmark of the fp8-activation projections (``--quantization ptpc_fp8``,
kernels/w8a8_gemm.hip) at the Llama-2-7B projection shapes, M = 1 .. 4096.  Per (shape, M) it
times, alternated within one process as lumen/bench/w8_bench.py does:

1. ``bf16``      the 16-bit ``linear_nt``;
2. ``fp8``       today's weight-only route (``linear_nt`` on an ``act=None`` QuantWeight);
3. ``w8a8_*``    every W8A8 candidate WITH its ``act_quant_fp8`` launch: the GEMV at M <= 4, each
                 compiled (BM, BN) x split-K x MFMA-form candidate of the decode kernel at
                 5 <= M <= 256, the block-tiled kernel above;
4. ``fallback``  the fake-quant fallback (activation quantizer, ``w8_dequant``, the 16-bit path,
                 the row scales).

and ``act_quant_fp8`` alone (GB/s).  Writes ``w8a8_bench.json``, a ``README.md`` table and the plan
table derived from it (``w8a8_gemm_plans.json``: a (N, K, bucket) is listed only where one candidate
beat the fallback at every measured M of the bucket) into ``--out``."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from lumen.bench.w8_bench import SHAPES, nbytes  # noqa: E402

MS = (1, 2, 4, 8, 16, 32, 64, 128, 192, 256, 512, 2048, 4096)
SPLITS = (1, 2, 4, 8)
ROUNDS = 5


def time_variants(variants, copies, reps):
    """{name: us per launch}: every variant warmed up, then ROUNDS rounds in which each variant
    runs ``reps`` launches back to back (variants alternated round by round); the median round."""
    import torch

    for fn in variants.values():
        for c in range(min(copies, 3)):
            fn(c)
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(reps):
                fn(i % copies)
            e1.record()
            e1.synchronize()
            rounds[name].append(e0.elapsed_time(e1) * 1e3 / reps)
    return {k: round(sorted(v)[len(v) // 2], 2) for k, v in rounds.items()}


def candidates(M, N, K):
    from lumen.ops.gemm import W8A8_BMS, W8A8_BNS, W8A8_FORMS

    bm = next(b for b in W8A8_BMS if M <= b)
    out = []
    for bn in W8A8_BNS[bm]:
        tiles = -(-N // bn)
        for s in SPLITS:
            # at most ~4 blocks per CU, at least 4 k128 steps per slice
            if s > 1 and (tiles * s > 1024 or -(-K // 128) // s < 4):
                continue
            out += [(bm, bn, s, f) for f in W8A8_FORMS]
    return out


def bucket_of(M):
    from lumen.ops.gemm import W8A8_BMS, w8a8_gemm_bucket

    return next(b for b in W8A8_BMS if M <= b) if M <= 256 else w8a8_gemm_bucket(M)


def derive_plans(rows, form):
    """One (BN, S) per (N, K, bucket): the candidate of MFMA form ``form`` (decode buckets) or
    the block-tiled kernel (large-M buckets) with the least total time over the bucket's measured
    M, listed only if it beat the fallback at every one of them."""
    buckets = {}
    for r in rows:
        if r["M"] <= 4:
            continue
        for name, us in r["us"].items():
            if name == "w8a8_gemm":
                key = (128, 1)
            elif name.startswith("w8a8_bm") and name.endswith(f"_f{form}"):
                _, bn, s, _ = (int(t.lstrip("bmnsf")) for t in name[5:].split("_"))
                key = (bn, s)
            else:
                continue
            buckets.setdefault((r["N"], r["K"], bucket_of(r["M"])), {}).setdefault(key, []).append(
                (r["M"], us, r["us"]["fallback"]))
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
        os.path.abspath(__file__)))), "profiles", "w8a8_serve"))
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--ms", default=",".join(map(str, MS)))
    ap.add_argument("--form", type=int, default=None,
                    help="MFMA form the plan table is derived for (default: lumen.ops.gemm.W8A8_FORM)")
    a = ap.parse_args()

    import torch

    import lumen.ops.gemm as gm
    from lumen.ops._native import native
    from lumen.ops.quant import QuantWeight, quantize_fp8_rows
    from lumen.utils.boxcal import box_record, fixed_work
    from lumen.utils.gemm_tuning import load_tuned_gemms

    if not torch.cuda.is_available() or native() is None:
        raise SystemExit("w8a8_bench needs a GPU and the native extension")
    load_tuned_gemms()
    dev = torch.device("cuda", 0)
    form = gm.W8A8_FORM if a.form is None else a.form
    os.makedirs(a.out, exist_ok=True)
    rows, quant = [], []
    for name in a.shapes.split(","):
        N, K = SHAPES[name]
        # rotate over enough weight copies that every call streams from HBM (> 256 MB MALL)
        copies = max(2, int(600e6 // (N * K)))
        w16 = [(torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16) for _ in range(copies)]
        w8 = [quantize_fp8_rows(w) for w in w16]
        wa = [QuantWeight(w.q, w.scale, w.dtype, act="fp8") for w in w8]
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
                        "fp8": lambda c: gm.linear_nt(x, w8[c]), "fallback": fallback}
            if M <= 4:
                variants["w8a8_gemv"] = lambda c: gm.w8a8_gemv(*gm.act_quant_fp8(x), wa[c], out=y)
            elif M <= 256:
                for bm, bn, s, f in candidates(M, N, K):
                    variants[f"w8a8_bm{bm}_bn{bn}_s{s}_f{f}"] = (
                        lambda c, bm=bm, bn=bn, s=s, f=f: gm.w8a8_decode_gemm(
                            *gm.act_quant_fp8(x), wa[c], bm, bn, s, f, out=y))
            else:
                variants["w8a8_gemm"] = lambda c: gm.w8a8_gemm(*gm.act_quant_fp8(x), wa[c], out=y)
            us = time_variants(variants, copies, 40 if M <= 256 else 10)
            row = {"shape": name, "N": N, "K": K, "M": M, "us": us,
                   "bytes": {"bf16": nbytes(M, N, K, 2), "fp8": nbytes(M, N, K, 1)}}
            if M > 256:
                row["TFLOPs"] = {k: round(2.0 * M * N * K / v / 1e6, 1) for k, v in us.items()}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del w16, w8, wa
        torch.cuda.empty_cache()
    # the activation quantizer alone: 2 bytes read + 1 byte written per element
    for K in sorted({SHAPES[n][1] for n in a.shapes.split(",")}):
        for M in (1, 16, 256, 4096):
            x = torch.randn(M, K, device=dev).to(torch.bfloat16)
            us = time_variants({"act_quant": lambda c: gm.act_quant_fp8(x)}, 1, 40)["act_quant"]
            quant.append({"M": M, "K": K, "us": us, "GBps": round(3.0 * M * K / us / 1e3, 1)})
            print(json.dumps(quant[-1]), flush=True)
    box = box_record(dev, {"launches_per_variant": "5 x 40 (M <= 256), 5 x 10 above"},
                     fixed_work(dev))
    plans = {f: derive_plans(rows, f) for f in gm.W8A8_FORMS}
    with open(os.path.join(a.out, "w8a8_bench.json"), "w") as f:
        json.dump({"box": box, "rows": rows, "act_quant": quant,
                   "plans_by_form": {str(k): v for k, v in plans.items()}}, f, indent=1)
    with open(os.path.join(a.out, "w8a8_gemm_plans.json"), "w") as f:
        json.dump({"source": "lumen/bench/w8a8_bench.py (profiles/w8a8_serve/w8a8_bench.json)",
                   "form": form, "plans": plans[form]}, f, indent=1)
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(table(rows, quant, box))
    print(json.dumps({"plans": {k: len(v) for k, v in plans.items()}, "out": a.out}), flush=True)


def table(rows, quant, box) -> str:
    fw = box.get("fixed_work", {})
    out = ["# fp8-activation (ptpc_fp8, W8A8) projections: measured (lumen/bench/w8a8_bench.py)", "",
           f"Box: {json.dumps(box.get('device'))}; fixed work: GEMM "
           f"{fw.get('gemm', {}).get('pflops')} PFLOP/s, HBM read "
           f"{fw.get('hbm_read', {}).get('tbps')} TB/s.", "",
           "us per call.  `bf16` is the 16-bit `linear_nt`, `fp8` the weight-only route, `best "
           "W8A8` the fastest W8A8 kernel candidate (f0: scaled K = 128 MFMA, f1: non-scaled "
           "K = 32 MFMA), `other form` the best candidate of the other MFMA form, `fallback` the "
           "fake-quant fallback.  The W8A8 and fallback times include the `act_quant_fp8` launch.",
           "",
           "| shape | M | bf16 | fp8 | best W8A8 | candidate | other form | fallback |",
           "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        k8 = {k: v for k, v in r["us"].items() if k.startswith("w8a8_")}
        best = min(k8, key=k8.get)
        other = {k: v for k, v in k8.items() if k[-3:-1] == "_f" and k[-1] != best[-1]}
        out.append(f"| {r['shape']} {r['N']}x{r['K']} | {r['M']} | {r['us']['bf16']} | "
                   f"{r['us']['fp8']} | {k8[best]} | {best} | "
                   f"{min(other.values()) if other else '-'} | {r['us']['fallback']} |")
    out += ["", "## act_quant_fp8 alone", "", "| M | K | us | GB/s (3 bytes per element) |",
            "|---|---|---|---|"]
    out += [f"| {q['M']} | {q['K']} | {q['us']} | {q['GBps']} |" for q in quant]
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main()
