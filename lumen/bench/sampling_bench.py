"""Sampler kernel benchmark: the per-row entry (kernels/sampling_rows.hip) next to ``sample`` and
to the host-side penalty path it replaces.  256 x 32000 bf16, T = 0.8, top-k 50, top-p 0.95.

  sample            the plain entry
  rows_off          sample_rows, nothing on (uniform seed / offset, rngrow = row)
  rows_on           sample_rows with penalties from the count table, 16 bias entries per row and
                    min_p 0.05
  rows_guided       sample_rows with every row guided: one 64-state token table (int16
                    [64, V], ~5 % of the tokens allowed in every state), the rows spread over
                    the states; the extra traffic is one table row per logits row (16.4 MB a
                    call at 256 x 32000)
  host_penalties    engine.apply_penalties on 256 sequences of 576 ids (512 prompt + 64
                    generated), then ``sample``: host wall time, ended by a synchronise

Kernel rows are device-event times over alternating repeats (median of ``--repeats`` windows of
``--iters`` calls).  Writes one JSON object (``--out``) and prints it.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import time


def main():
    import torch

    from lumen.ops._native import native
    from lumen.serve.engine import apply_penalties
    from lumen.serve.sequence import SamplingParams, Sequence

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sampling_bench needs a GPU")
    C = native()
    assert C is not None
    dev = "cuda"
    R, V = a.rows, a.vocab
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(R, V, generator=g) * 3).to(torch.bfloat16).to(dev)
    temp = torch.full((R,), 0.8, device=dev)
    top_p = torch.full((R,), 0.95, device=dev)
    top_k = torch.full((R,), 50, device=dev, dtype=torch.int32)
    out = torch.empty(R, device=dev, dtype=torch.int64)
    lp = torch.empty(R, device=dev, dtype=torch.float32)
    seed = torch.full((R,), 7, device=dev, dtype=torch.int64)
    offset = torch.full((R,), 3, device=dev, dtype=torch.int64)
    rngrow = torch.arange(R, device=dev)
    # 576 ids a sequence: 512 prompt + 64 generated
    prompt = torch.randint(3, V, (R, 512), generator=g)
    gen = torch.randint(3, V, (R, 64), generator=g)
    counts = torch.zeros(R, V, dtype=torch.int32, device=dev)
    slots = torch.arange(R, device=dev, dtype=torch.int32)
    ptr = (torch.arange(R + 1) * 576).to(torch.int32).to(dev)
    C.sampler_state_init(counts, slots, ptr, torch.full((R,), 512, dtype=torch.int32, device=dev),
                         torch.cat([prompt, gen], 1).reshape(-1).to(torch.int32).to(dev), R)
    counts0 = counts.clone()
    nb = 16
    bias_ptr = (torch.arange(R + 1) * nb).to(torch.int32).to(dev)
    bias_idx = torch.randint(3, V, (R * nb,), generator=g).to(torch.int32).to(dev)
    bias_val = (torch.randn(R * nb, generator=g) * 2).to(dev)
    min_p = torch.full((R,), 0.05, device=dev)
    rp = torch.full((R,), 1.1, device=dev)
    fp = torch.full((R,), 0.5, device=dev)
    pp = torch.full((R,), 0.2, device=dev)
    # guided rows: a 64-state table, ~5 % of the tokens allowed, successors anywhere
    GS = 64
    g_next = torch.where(torch.rand(GS, V, generator=g) < 0.05,
                         torch.randint(0, GS, (GS, V), generator=g), torch.tensor(-1))
    g_next = g_next.to(torch.int16).to(dev)
    g_table = torch.full((R,), g_next.data_ptr(), device=dev, dtype=torch.int64)
    g_state = (torch.arange(R) % GS).to(torch.int32).to(dev)
    seqs = []
    for i in range(R):
        s = Sequence(prompt[i].tolist(), SamplingParams(frequency_penalty=0.5, presence_penalty=0.2,
                                                        repetition_penalty=1.1))
        s.output_ids = gen[i].tolist()
        seqs.append(s)

    def k_sample():
        C.sample(logits, temp, top_p, top_k, 7, 3, out, lp)

    def k_off():
        C.sample_rows(logits, temp, top_p, top_k, seed, offset, rngrow, out_tokens=out,
                      out_logprob=lp)

    def k_on():
        C.sample_rows(logits, temp, top_p, top_k, seed, offset, rngrow, min_p=min_p,
                      bias_ptr=bias_ptr, bias_idx=bias_idx, bias_val=bias_val, slot=slots, rp=rp,
                      fp=fp, pp=pp, counts=counts, out_tokens=out, out_logprob=lp)

    def k_guided():
        C.sample_rows(logits, temp, top_p, top_k, seed, offset, rngrow, out_tokens=out,
                      out_logprob=lp, g_table=g_table, g_slot=slots, g_state=g_state)

    def k_host():
        C.sample(apply_penalties(logits, seqs), temp, top_p, top_k, 7, 3, out, lp)

    kernels = {"sample": k_sample, "rows_off": k_off, "rows_on": k_on, "rows_guided": k_guided}
    for f in list(kernels.values()) + [k_host]:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in kernels}
    for _ in range(a.repeats):          # alternate the variants: drift hits them alike
        for name, f in kernels.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                f()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1000.0 / a.iters)
        counts.copy_(counts0)           # rows_on advances the table: start every window alike
    host = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k_host()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e6)
    res = {"rows": R, "vocab": V, "dtype": "bf16", "temperature": 0.8, "top_k": 50, "top_p": 0.95,
           "iters": a.iters, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0),
           "us_per_call": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2),
                               "max": round(max(v), 2)} for k, v in times.items()},
           "host_penalties_us_per_call": {"median": round(statistics.median(host), 1),
                                          "min": round(min(host), 1), "max": round(max(host), 1)},
           "state_table_mb": round(counts.numel() * 4 / 1e6, 1),
           "guided_table_states": GS, "guided_allowed_fraction": 0.05,
           "guided_table_bytes_read_per_call": R * V * 2}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
