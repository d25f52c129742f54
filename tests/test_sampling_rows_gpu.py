"""The per-row sampler entry (kernels/sampling_rows.hip) and the engine's device sampler state:
per-request seeds, min_p, logit_bias, penalties from the count table, the count update and the
state init kernel, against torch references; then the engine paths on the tiny model."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32


@pytest.fixture(autouse=True)
def _native():
    from lumen.ops._native import native, native_error

    assert native() is not None, f"native extension must load on the GPU box: {native_error()!r}"
    torch.manual_seed(0)


def _C():
    from lumen.ops._native import native

    return native()


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32, device=DEV)


def _f32(x):
    return torch.as_tensor(x, dtype=F32, device=DEV)


def _i64(x):
    return torch.as_tensor(x, dtype=torch.int64, device=DEV)


def _ulp(m: torch.Tensor) -> torch.Tensor:
    """One f32 unit in the last place at magnitude m (f64 tensor)."""
    e = torch.floor(torch.log2(m.clamp(min=2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 23)


def _rows_call(logits, temp, top_p, top_k, seed, offset, rngrow, want_tau=True, **kw):
    R = logits.shape[0]
    out = torch.empty(R, device=DEV, dtype=torch.int64)
    lp = torch.empty(R, device=DEV, dtype=F32)
    tau = torch.empty(R, device=DEV, dtype=F32) if want_tau else None
    _C().sample_rows(logits, temp, top_p, top_k, seed, offset, rngrow, out_tokens=out,
                     out_logprob=lp, out_tau=tau, **kw)
    return out, lp, tau


# ---- identity with the old entry ------------------------------------------------------------
@pytest.mark.parametrize("R,V,dtype", [(6, 32000, F32), (6, 32000, torch.bfloat16), (4, 512, F32),
                                       (3, 515, torch.bfloat16), (2, 40000, torch.bfloat16)])
@pytest.mark.parametrize("greedy", [True, False])
def test_rows_entry_equals_sample(R, V, dtype, greedy):
    """Uniform seed / offset, rngrow = the row and nothing else on: the tokens and thresholds
    of ``sample``, bit for bit (LDS rows, unaligned rows, the no-LDS route)."""
    g = torch.Generator().manual_seed(R * 31 + V)
    logits = (torch.randn(R, V, generator=g) * 3).to(dtype).to(DEV)
    temp = torch.full((R,), 0.0 if greedy else 0.7, device=DEV)
    top_p = torch.full((R,), 1.0 if greedy else 0.9, device=DEV)
    top_k = torch.full((R,), 0 if greedy else 50, device=DEV, dtype=torch.int32)
    out0 = torch.empty(R, device=DEV, dtype=torch.int64)
    lp0 = torch.empty(R, device=DEV, dtype=F32)
    tau0 = torch.empty(R, device=DEV, dtype=F32)
    _C().sample(logits, temp, top_p, top_k, 5, 3, out0, lp0, tau0)
    out, lp, tau = _rows_call(logits, temp, top_p, top_k, _i64([5] * R), _i64([3] * R),
                              torch.arange(R, device=DEV))
    assert torch.equal(out, out0)
    assert torch.equal(tau, tau0)
    torch.testing.assert_close(lp, lp0)
    # the same with every optional argument present but off
    S = 2
    counts = torch.zeros(S, V, dtype=torch.int32, device=DEV)
    out, lp, tau = _rows_call(
        logits, temp, top_p, top_k, _i64([5] * R), _i64([3] * R), torch.arange(R, device=DEV),
        min_p=torch.zeros(R, device=DEV), bias_ptr=_i32([0] * (R + 1)), bias_idx=_i32([]),
        bias_val=_f32([]), slot=_i32([-1] * R), rp=torch.ones(R, device=DEV),
        fp=torch.zeros(R, device=DEV), pp=torch.zeros(R, device=DEV), counts=counts)
    assert torch.equal(out, out0) and torch.equal(tau, tau0)
    assert int(counts.abs().sum()) == 0


def test_row_position_invariance():
    """One logits row at rows 0, 3 and 7 of a batch with the same (seed, offset, rngrow = 0):
    the same token each time; another offset gives other draws."""
    R, V = 8, 32000
    g = torch.Generator().manual_seed(21)
    logits = (torch.randn(R, V, generator=g) * 3).to(DEV)
    logits[3] = logits[0]
    logits[7] = logits[0]
    temp = torch.ones(R, device=DEV)
    top_p = torch.ones(R, device=DEV)
    top_k = torch.zeros(R, device=DEV, dtype=torch.int32)
    seed = _i64([77, 1, 2, 77, 3, 4, 5, 77])
    offset = _i64([9, 0, 1, 9, 2, 3, 4, 9])
    rngrow = _i64([0, 1, 2, 0, 4, 5, 6, 0])
    out, _, _ = _rows_call(logits, temp, top_p, top_k, seed, offset, rngrow)
    assert out[0] == out[3] == out[7]
    # 32 rows drawn at offset 4 and at offset 5
    R = 32
    logits = (torch.randn(R, V, generator=g) * 3).to(DEV)
    temp, top_p = torch.ones(R, device=DEV), torch.ones(R, device=DEV)
    top_k = torch.zeros(R, device=DEV, dtype=torch.int32)
    zero = _i64([0] * R)
    a, _, _ = _rows_call(logits, temp, top_p, top_k, _i64([77] * R), _i64([4] * R), zero)
    a2, _, _ = _rows_call(logits, temp, top_p, top_k, _i64([77] * R), _i64([4] * R), zero)
    b, _, _ = _rows_call(logits, temp, top_p, top_k, _i64([77] * R), _i64([5] * R), zero)
    assert torch.equal(a, a2)
    assert bool((a != b).any())


# ---- logits_process / fused greedy against an f64 reference -----------------------------------
_PROC = {}


def _proc_case(V, dtype):
    """Inputs and the f64 reference of one (V, dtype) case, built once and shared."""
    key = (V, dtype)
    if key in _PROC:
        return _PROC[key]
    R, S = 5, 4
    g = torch.Generator().manual_seed(V + {F32: 0, torch.bfloat16: 1, torch.float16: 2}[dtype])
    logits = (torch.randn(R, V, generator=g) * 3).clamp(-64, 64).to(dtype)
    # count rows: prompt-only, generated-only and both-bits tokens, most tokens unseen
    kind = torch.randint(0, 10, (S, V), generator=g)
    n = torch.randint(1, 6, (S, V), generator=g)
    c64 = torch.zeros(S, V, dtype=torch.int64)
    c64 = torch.where(kind == 0, torch.full_like(c64, 1 << 31), c64)
    c64 = torch.where(kind == 1, n, c64)
    c64 = torch.where(kind == 2, n + (1 << 31), c64)
    counts = torch.where(c64 >= (1 << 31), c64 - (1 << 32), c64).to(torch.int32)
    slot = torch.tensor([2, 0, -1, 3, 1])
    rp = torch.tensor([1.3, 1.0, 1.3, 1.3, 1.0], dtype=F32)
    fp = torch.tensor([0.7, -0.5, 0.7, 0.0, 0.0], dtype=F32)
    pp = torch.tensor([0.0, 0.7, -0.5, -0.5, 0.0], dtype=F32)
    ninf = -float("inf")
    bias = [([1, 7, V - 1, 100], [5.0, ninf, -2.5, 100.0]), None,
            ([0, 3], [-100.0, 1.25]), ([2, 9, 11, 200, 201], [ninf, 0.5, -0.75, 3.0, -3.0]), None]
    ptr, idx, val = [0], [], []
    for e in bias:
        if e is not None:
            idx += e[0]
            val += e[1]
        ptr.append(len(idx))
    # f64 reference, step by step, with the largest intermediate magnitude of every element
    x0 = logits.double()
    b = torch.zeros(R, V, dtype=torch.float64)
    hasb = torch.zeros(R, V, dtype=torch.bool)
    for i, e in enumerate(bias):
        if e is not None:
            b[i, e[0]] = torch.tensor(e[1], dtype=F32).double()
            hasb[i, e[0]] = True
    x1 = x0 + b
    c = torch.zeros(R, V, dtype=torch.int64)
    for i in range(R):
        if slot[i] >= 0:
            c[i] = c64[slot[i]]
    nn = (c & 0x7FFFFFFF).double()
    rpd, fpd, ppd = rp.double()[:, None], fp.double()[:, None], pp.double()[:, None]
    x2 = torch.where((c != 0) & (rpd != 1.0), torch.where(x1 > 0, x1 / rpd, x1 * rpd), x1)
    pen = fpd * nn + ppd * (nn > 0).double()
    x3 = torch.where(c != 0, x2 - pen, x2)
    fin = torch.isfinite(x3)
    mag = torch.stack([t.abs() for t in (x0, torch.where(fin, x1, x0), torch.where(fin, x2, x0),
                                         (fpd * nn).abs(), pen, torch.where(fin, x3, x0))]).amax(0)
    case = dict(R=R, S=S, logits=logits.to(DEV), counts=counts.to(DEV), slot=_i32(slot),
                rp=rp.to(DEV), fp=fp.to(DEV), pp=pp.to(DEV), bias=bias,
                bias_ptr=_i32(ptr), bias_idx=_i32(idx), bias_val=_f32(val),
                ref=x3, touched=hasb | (c != 0), tol=4 * _ulp(mag), c=c)
    _PROC[key] = case
    return case


@pytest.mark.parametrize("dtype", [F32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("V", [512, 515, 32000, 40000])
def test_logits_process_vs_f64(V, dtype):
    """Bias, then repetition on the biased sign, then frequency / presence: untouched elements
    bit-equal to float(logit); touched ones within 4 f32 ulp of the largest intermediate
    magnitude (at most three f32 operations, the multiply-add possibly contracted)."""
    from lumen.serve.model_runner import process_logits_ref

    k = _proc_case(V, dtype)
    out = torch.empty(k["R"], V, device=DEV, dtype=F32)
    _C().logits_process(k["logits"], k["bias_ptr"], k["bias_idx"], k["bias_val"], k["slot"],
                        k["rp"], k["fp"], k["pp"], k["counts"], out)
    got = out.cpu()
    x0 = k["logits"].float().cpu()
    un = ~k["touched"]
    assert torch.equal(got[un], x0[un])
    ref = k["ref"]
    inf = ~torch.isfinite(ref)
    assert int(inf.sum()) == 2 and torch.equal(got[inf].double(), ref[inf])
    err = (got.double() - ref).abs()[~inf]
    tol = k["tol"][~inf]
    worst = (err / tol).max().item()
    print(f"logits_process V={V} {dtype}: worst error {worst:.3f} of the 4-ulp bound")
    assert bool((err <= tol).all()), worst
    # the library's torch reference is the same function
    counts_rows = torch.zeros(k["R"], V, dtype=torch.int64)
    counts_rows[:] = k["c"]
    lib = process_logits_ref(k["logits"].double().cpu(), counts_rows, k["rp"].cpu(), k["fp"].cpu(),
                             k["pp"].cpu(), bias=[None if e is None else
                                                  (e[0], torch.tensor(e[1], dtype=F32))
                                                  for e in k["bias"]])
    assert torch.equal(torch.nan_to_num(lib, neginf=-1e300), torch.nan_to_num(ref, neginf=-1e300))


@pytest.mark.parametrize("dtype", [F32, torch.bfloat16])
@pytest.mark.parametrize("V", [512, 515, 32000, 40000])
def test_fused_greedy_equals_reference_argmax(V, dtype):
    """Greedy ``sample_rows`` with bias and penalties in the launch = argmax of the f64
    reference (its top-2 gap is wider than the error bound, asserted)."""
    k = _proc_case(V, dtype)
    R = k["R"]
    ref = k["ref"]
    top2 = ref.topk(2, -1).values
    gap = top2[:, 0] - top2[:, 1]
    am = ref.argmax(-1)
    bound = 2 * k["tol"].gather(1, ref.topk(2, -1).indices).amax(-1)
    assert bool((gap > bound).all()), (gap, bound)
    before = k["counts"].clone()
    counts = k["counts"].clone()
    out, _, _ = _rows_call(k["logits"], torch.zeros(R, device=DEV), torch.ones(R, device=DEV),
                           torch.zeros(R, device=DEV, dtype=torch.int32), _i64([1] * R),
                           _i64([0] * R), torch.arange(R, device=DEV),
                           bias_ptr=k["bias_ptr"], bias_idx=k["bias_idx"], bias_val=k["bias_val"],
                           slot=k["slot"], rp=k["rp"], fp=k["fp"], pp=k["pp"], counts=counts)
    assert torch.equal(out.cpu(), am)
    # and the counts of the chosen tokens advanced, nothing else
    for r in range(R):
        s = int(k["slot"][r])
        if s >= 0:
            before[s, am[r]] += 1
    assert torch.equal(counts, before)
    # pre = True over the materialised rows: the same tokens, the counts advance exactly once
    x = torch.empty(R, V, device=DEV, dtype=F32)
    _C().logits_process(k["logits"], k["bias_ptr"], k["bias_idx"], k["bias_val"], k["slot"],
                        k["rp"], k["fp"], k["pp"], k["counts"], x)
    counts2 = k["counts"].clone()
    out2, _, _ = _rows_call(x, torch.zeros(R, device=DEV), torch.ones(R, device=DEV),
                            torch.zeros(R, device=DEV, dtype=torch.int32), _i64([1] * R),
                            _i64([0] * R), torch.arange(R, device=DEV), slot=k["slot"],
                            rp=k["rp"], fp=k["fp"], pp=k["pp"], counts=counts2, pre=True)
    assert torch.equal(out2.cpu(), am) and torch.equal(counts2, before)


@pytest.mark.parametrize("V", [515, 32000, 40000])
def test_count_update(V):
    """One call: counts[slot[r], tok[r]] rises by exactly one for rows with a slot; the rest of
    the table, and every row of a slot-less sequence, is unchanged."""
    R, S = 6, 5
    g = torch.Generator().manual_seed(V)
    logits = (torch.randn(R, V, generator=g) * 3).to(torch.bfloat16).to(DEV)
    counts = torch.randint(0, 4, (S, V), generator=g).to(torch.int32).to(DEV)
    before = counts.clone()
    slot = [3, -1, 0, 4, -1, 1]
    out, _, _ = _rows_call(logits, torch.full((R,), 0.8, device=DEV), torch.ones(R, device=DEV),
                           torch.zeros(R, device=DEV, dtype=torch.int32), _i64([3] * R),
                           _i64([2] * R), torch.arange(R, device=DEV), slot=_i32(slot),
                           rp=torch.full((R,), 1.1, device=DEV), fp=torch.full((R,), 0.2, device=DEV),
                           pp=torch.zeros(R, device=DEV), counts=counts)
    for r, s in enumerate(slot):
        if s >= 0:
            before[s, out[r]] += 1
    assert torch.equal(counts, before)
    assert torch.equal(counts[2], before[2])   # a slot no row owns


@pytest.mark.parametrize("V", [512, 515])
def test_sampler_state_init(V):
    """The slot row = the scatter of the ids (bit 31 for the prompt, counts for the generated
    ones; duplicates, an id equal to V and a negative id skipped); a dirty row comes out clean,
    other slots stay."""
    S = 4
    g = torch.Generator().manual_seed(V)
    counts = torch.randint(-5, 9, (S, V), generator=g).to(torch.int32).to(DEV)
    before = counts.clone().cpu()
    seqs = {2: ([3, 3, 7, V, 9, -1, V - 1], [7, 7, 11, 3, V, -4, V - 1, 11, 11]),
            0: ([5], []), 3: ([], [1, 1, 2])}
    slots, ptr, npr, ids = [], [0], [], []
    for s, (p, o) in seqs.items():
        slots.append(s)
        npr.append(len(p))
        ids += p + o
        ptr.append(len(ids))
    _C().sampler_state_init(counts, _i32(slots), _i32(ptr), _i32(npr), _i32(ids), len(slots))
    exp = before.clone()
    for s, (p, o) in seqs.items():
        row = torch.zeros(V, dtype=torch.int64)
        for t in p:
            if 0 <= t < V:
                row[t] |= 1 << 31
        for t in o:
            if 0 <= t < V:
                row[t] += 1
        exp[s] = torch.where(row >= (1 << 31), row - (1 << 32), row).to(torch.int32)
    assert torch.equal(counts.cpu(), exp)
    assert torch.equal(counts[1].cpu(), before[1])


# ---- min_p --------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_p", [0.01, 0.05, 0.2])
@pytest.mark.parametrize("T", [1.0, 0.5])
@pytest.mark.parametrize("dtype", [F32, torch.bfloat16])
def test_min_p_kept_set(dtype, T, min_p):
    """The kept set the kernel reports (out_tau) = z >= max(z) + ln(min_p); tokens within 4 ulp
    of the threshold may fall either way (fewer than 1 % of the kept ones are that close).  With
    top_k = 50 as well: the intersection."""
    from lumen.serve.model_runner import min_p_keep, topk_topp_keep

    R, V = 8, 32000
    g = torch.Generator(device="cpu").manual_seed(int(min_p * 1000) + int(T * 10))
    logits = (torch.randn(R, V, generator=g) * 3.0).to(dtype).to(DEV)
    temp = torch.full((R,), T, device=DEV)
    mp = torch.full((R,), min_p, device=DEV)
    common = (_i64([5] * R), _i64([1] * R), torch.arange(R, device=DEV))
    out, _, tau = _rows_call(logits, temp, torch.ones(R, device=DEV),
                             torch.zeros(R, device=DEV, dtype=torch.int32), *common, min_p=mp)
    outk, _, tauk = _rows_call(logits, temp, torch.ones(R, device=DEV),
                               torch.full((R,), 50, device=DEV, dtype=torch.int32), *common,
                               min_p=mp)
    for i in range(R):
        zs = logits[i].float() * (1.0 / temp[i])
        m = zs.max().double()
        thr = m + math.log(min_p)
        band = (zs.double() - thr).abs() <= 4 * _ulp(torch.maximum(m.abs(), thr.abs()).cpu()).to(DEV)
        ref = min_p_keep(zs, min_p)
        kept = zs >= tau[i]
        assert int(band.sum()) < 0.01 * int(ref.sum()), (int(band.sum()), int(ref.sum()))
        assert torch.equal(kept[~band], ref[~band]), (i, int(kept.sum()), int(ref.sum()))
        assert kept[out[i]]
        refk = ref & topk_topp_keep(zs, 50, 1.0)
        keptk = zs >= tauk[i]
        assert torch.equal(keptk[~band], refk[~band]), (i, int(keptk.sum()), int(refk.sum()))
        assert keptk[outk[i]]


def test_min_p_distribution_chi2_per_row_seeds():
    """65,536 rows of one V = 200 distribution, each with its own seed (rngrow = 0), min_p 0.05
    at temperature 0.8: nothing outside the kept set, and a chi-square test of the counts
    against the renormalised truncated distribution -- per-row seeding is still a fair draw."""
    from scipy.stats import chisquare

    from lumen.serve.model_runner import min_p_keep

    R, V = 65536, 200
    g = torch.Generator(device="cpu").manual_seed(3)
    row = torch.randn(V, generator=g) * 2.0
    logits = row.expand(R, V).contiguous().to(DEV)
    T = 0.8
    out, _, _ = _rows_call(logits, torch.full((R,), T, device=DEV), torch.ones(R, device=DEV),
                           torch.zeros(R, device=DEV, dtype=torch.int32),
                           torch.arange(R, device=DEV) + 1000, _i64([9] * R), _i64([0] * R),
                           want_tau=False, min_p=torch.full((R,), 0.05, device=DEV))
    zs = row.float() * (1.0 / torch.tensor(T, dtype=F32))
    keep = min_p_keep(zs, 0.05)
    cnt = torch.bincount(out.cpu(), minlength=V).double()
    assert cnt[~keep].sum() == 0
    pr = torch.softmax(zs.double(), -1)[keep]
    exp = pr / pr.sum() * R
    res = chisquare(cnt[keep].numpy(), exp.numpy())
    assert res.pvalue > 1e-4, (res, int(keep.sum()))


# ---- engine ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from lumen.models import build_model

    m = build_model("tiny-llama-gqa", dtype=torch.bfloat16, device="cuda", init="random", seed=1)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 2:
                p.mul_(5.0)
    return m.eval()


def _engine(model, **kw):
    from lumen.serve.engine import EngineConfig, LLMEngine

    kw.setdefault("num_blocks", 128)
    kw.setdefault("use_graphs", False)
    return LLMEngine(EngineConfig(model="tiny-llama-gqa", device="cuda", max_model_len=512,
                                  block_size=16, **kw), model=model)


def test_engine_seed_reproducible_async(model):
    from lumen.serve.sequence import SamplingParams

    prompt = [17, 4, 99, 23, 8]
    sp = dict(max_tokens=12, temperature=1.0, ignore_eos=True, seed=11)
    other = lambda n: SamplingParams(max_tokens=n, temperature=1.0, ignore_eos=True)  # noqa: E731

    def run(before, after_steps=0):
        eng = _engine(model, async_scheduling=True)
        for ids, n in before:
            eng.add_request(ids, other(n))
        for _ in range(after_steps):
            eng.step()
        s = eng.add_request(prompt, SamplingParams(**sp))
        while eng.has_work:
            eng.step()
        assert eng.async_sched and eng.stats["overlapped_steps"] > 0
        return s.output_ids

    alone = run([])
    assert len(alone) == 12
    assert run([([3, 4, 5], 12), ([9, 9, 9, 9], 12)]) == alone
    assert run([([3, 4, 5], 3), ([9, 9, 9, 9], 20), ([40, 41], 7), ([50], 5), ([60, 61, 62], 9)],
               after_steps=3) == alone


def _run_penalised(model, pen, num_blocks=128, graphs=False, stop_case=False):
    from lumen.serve.sequence import SamplingParams

    eng = _engine(model, async_scheduling=True, num_blocks=num_blocks, use_graphs=graphs,
                  max_num_seqs=8)
    eng.blocks.watermark_blocks = 0
    prompts = [[5, 5, 5, 5] * 6, [9, 8, 7] * 9, list(range(3, 40)), [42, 43] * 12]
    kw = dict(frequency_penalty=1.5, repetition_penalty=1.2) if pen else {}
    stop = dict(stop_case) if stop_case else {}
    if "eos" in stop:
        eng.eos_id = stop["eos"]
    seqs = []
    for i, p in enumerate(prompts):
        extra = {}
        if stop and i == 0:
            extra = dict(stop_token_ids=[stop["stop"]])
        elif not stop or i == 3:
            extra = dict(ignore_eos=True)
        seqs.append(eng.add_request(p, SamplingParams(max_tokens=40, temperature=0.0, **kw,
                                                      **extra)))
    while eng.has_work:
        eng.step()
    assert eng.blocks.num_free == eng.blocks.num_blocks
    assert eng.sampler_state.num_free == 8 and all(s.state_slot == -1 for s in seqs)
    assert all(s.n_pending == 0 for s in seqs)
    return eng, seqs


def test_engine_penalties_keep_async_overlap(model, monkeypatch):
    """Penalised greedy requests under async scheduling: the tokens of the host path
    (LUMEN_SAMPLER_STATE=0), with the overlap of an unpenalised run -- the count table lives on
    the device, no step waits for token values."""
    eng, dev = _run_penalised(model, True, graphs=True)
    assert eng.dev_state and eng.sampler_state.allocated
    plain_eng, plain = _run_penalised(model, False, graphs=True)
    assert not plain_eng.sampler_state.allocated       # no penalty seen: nothing allocated
    monkeypatch.setenv("LUMEN_SAMPLER_STATE", "0")
    host_eng, host = _run_penalised(model, True, graphs=True)
    monkeypatch.delenv("LUMEN_SAMPLER_STATE")
    assert not host_eng.dev_state and not host_eng.sampler_state.allocated
    for a, b in zip(dev, host):
        assert a.output_ids == b.output_ids
    assert any(a.output_ids != b.output_ids for a, b in zip(dev, plain))   # penalties act
    ov, ov_plain, ov_host = (e.stats["overlapped_steps"] for e in (eng, plain_eng, host_eng))
    print(f"overlapped steps: device state {ov}, no penalties {ov_plain}, host path {ov_host}")
    assert abs(ov - ov_plain) <= 2
    assert ov_host <= 3


def test_engine_penalties_stop_hit_in_flight(model, monkeypatch):
    """A stop id / EOS found while the next step is in flight (its row for the finished
    sequence is wasted, and may still bump the freed slot's counts): same tokens as the host
    path, every block and slot returned."""
    _, ref = _run_penalised(model, True)
    stop = dict(stop=ref[0].output_ids[3], eos=ref[1].output_ids[6])
    _, dev = _run_penalised(model, True, stop_case=stop)
    monkeypatch.setenv("LUMEN_SAMPLER_STATE", "0")
    _, host = _run_penalised(model, True, stop_case=stop)
    for a, b in zip(dev, host):
        assert a.output_ids == b.output_ids and a.finish_reason == b.finish_reason
    assert dev[0].finish_reason == "stop" and dev[0].output_ids[-1] == stop["stop"]


def test_engine_penalties_preemption(model):
    """A cache too small for the four sequences: a preempted sequence returns its slot and its
    counts are rebuilt from its host ids at re-admission -- the tokens of the roomy run."""
    _, ref = _run_penalised(model, True)
    eng, tight = _run_penalised(model, True, num_blocks=12)
    assert eng.scheduler.num_preemptions > 0
    for a, b in zip(tight, ref):
        assert a.output_ids == b.output_ids


def test_engine_slot_reuse(model):
    """More penalised requests than max_num_seqs = 2, one after another through the same two
    slots: each one's tokens equal its solo run."""
    from lumen.serve.sequence import SamplingParams

    sp = dict(max_tokens=16, temperature=0.0, ignore_eos=True, frequency_penalty=1.5,
              repetition_penalty=1.2, presence_penalty=0.5)
    prompts = [[5, 5, 5, 5], [9, 8, 7, 9, 8], list(range(3, 20)), [42, 43] * 4, [100] * 7]
    eng = _engine(model, async_scheduling=True, max_num_seqs=2)
    seqs = [eng.add_request(p, SamplingParams(**sp)) for p in prompts]
    while eng.has_work:
        eng.step()
    assert eng.sampler_state.num_free == 2
    solo_eng = _engine(model, async_scheduling=True, max_num_seqs=2)
    for p, s in zip(prompts, seqs):
        solo = solo_eng.generate([p], SamplingParams(**sp))[0]
        assert s.output_ids == solo.output_ids, p


def test_engine_top_logprobs_read_processed_logits(model):
    """top_logprobs with a bias and a penalty: the alternatives come from the logits the token
    was drawn from (the forced token leads them), and the counts advance once per token."""
    from lumen.serve.sequence import SamplingParams

    eng = _engine(model)
    s = eng.add_request([5, 9, 33, 7], SamplingParams(
        max_tokens=5, temperature=0.0, ignore_eos=True, top_logprobs=3, logit_bias={123: 100.0},
        frequency_penalty=0.5))
    slot_counts = None
    while eng.has_work:
        eng.step()
        if s.state_slot >= 0:
            slot_counts = eng.sampler_state.counts[s.state_slot].clone()
    assert s.output_ids == [123] * 5
    assert all(t[0][0] == 123 for t in s.output_top_logprobs)
    assert int(slot_counts[123]) == 4   # read before the last step's release: 4 tokens so far
