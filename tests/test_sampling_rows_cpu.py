"""Per-request seeds, min_p, logit_bias, min_tokens and the penalty reference on the CPU engine
(torch reference paths of kernels/sampling_rows.hip)."""
import math

import pytest
import torch

from lumen.models import build_model
from lumen.serve.engine import EngineConfig, LLMEngine, apply_penalties
from lumen.serve.model_runner import min_p_keep, process_logits_ref
from lumen.serve.sampler_state import counts_from_ids
from lumen.serve.sequence import SamplingParams, Sequence


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    m = build_model("tiny-llama-gqa", dtype=torch.float32, device="cpu", init="random", seed=1)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 2:
                p.mul_(5.0)
    m.eval()
    return m


def _engine(model, **kw):
    cfg = EngineConfig(model="tiny-llama-gqa", device="cpu", max_model_len=256, block_size=4,
                       use_graphs=False, num_blocks=400, **kw)
    return LLMEngine(cfg, model=model)


def test_params_construct_and_validate():
    p = SamplingParams(min_p=0.1, logit_bias={5: 2.5, "7": -100}, min_tokens=3)
    assert p.min_p == 0.1 and p.logit_bias == {5: 2.5, 7: -100.0} and p.min_tokens == 3
    assert p.row_features and not SamplingParams().row_features
    # the front-end hop: a params object rebuilt from its own fields
    assert SamplingParams(**vars(p)) == p
    for bad in (dict(min_p=-0.1), dict(min_p=1.5), dict(min_tokens=-1),
                dict(min_tokens=17, max_tokens=16), dict(logit_bias={3: 101.0}),
                dict(logit_bias={3: -100.5}), dict(logit_bias={-1: 1.0}),
                dict(logit_bias={"x": 1.0}), dict(logit_bias={i: 1.0 for i in range(301)})):
        with pytest.raises(ValueError):
            SamplingParams(**bad)


def test_api_accepts_and_rejects(model):
    from starlette.testclient import TestClient

    from lumen.serve.api_server import create_app
    from lumen.serve.engine import AsyncEngine

    eng = _engine(model)
    V = eng.model_config.vocab_size
    ae = AsyncEngine(eng)
    try:
        c = TestClient(create_app(ae, "tiny"))
        base = {"prompt": [5, 6, 7], "max_tokens": 4, "temperature": 0, "ignore_eos": True}
        r = c.post("/v1/completions", json=dict(base, logit_bias={"9": 100}, min_p=0.2,
                                                 min_tokens=2))
        assert r.status_code == 200, r.text
        assert r.json()["usage"]["completion_tokens"] == 4
        for bad in (dict(min_p=1.5), dict(min_p=-1), dict(min_tokens=9), dict(min_tokens=-1),
                    dict(logit_bias={"9": 101}), dict(logit_bias={"nine": 1}),
                    dict(logit_bias=[1, 2]), dict(logit_bias={str(V): 1.0}),
                    dict(logit_bias={str(V + 7): -5.0})):
            r = c.post("/v1/completions", json=dict(base, **bad))
            assert r.status_code == 400, (bad, r.status_code, r.text)
        assert c.post("/v1/completions", json=dict(base, logit_bias={str(V - 1): 1.0})
                      ).status_code == 200
    finally:
        ae.shutdown()
    assert eng.blocks.num_free == eng.blocks.num_blocks


@pytest.mark.parametrize("async_", [False, True])
def test_seed_is_reproducible_whatever_else_runs(model, async_):
    """A request with a seed gives the same tokens alone, behind other requests in the batch
    (not row 0), and among a different set of requests that finish at different times (other
    rows, other step counts)."""
    prompt = [17, 4, 99, 23, 8]
    sp = dict(max_tokens=12, temperature=1.0, ignore_eos=True, seed=11)
    other = lambda n: SamplingParams(max_tokens=n, temperature=1.0, ignore_eos=True)  # noqa: E731

    def run(before, after_steps=0):
        eng = _engine(model, async_scheduling=async_)
        for ids, n in before:
            eng.add_request(ids, other(n))
        for _ in range(after_steps):
            eng.step()
        s = eng.add_request(prompt, SamplingParams(**sp))
        while eng.has_work:
            eng.step()
        assert eng.async_sched == async_
        return s.output_ids

    alone = run([])
    assert len(alone) == 12
    assert run([([3, 4, 5], 12), ([9, 9, 9, 9], 12)]) == alone
    assert run([([3, 4, 5], 3), ([9, 9, 9, 9], 20), ([40, 41], 7), ([50], 5), ([60, 61, 62], 9)],
               after_steps=3) == alone
    # and the seed matters: another seed gives other tokens
    eng = _engine(model, async_scheduling=async_)
    assert eng.generate([prompt], SamplingParams(**dict(sp, seed=12)))[0].output_ids != alone


def test_logit_bias_forces_and_removes(model):
    eng = _engine(model)
    base = dict(max_tokens=8, temperature=0.0, ignore_eos=True)
    ref = eng.generate([[5, 9, 33, 7]], SamplingParams(**base))[0].output_ids
    t = 123
    out = eng.generate([[5, 9, 33, 7]], SamplingParams(logit_bias={t: 100.0}, **base))[0]
    assert out.output_ids == [t] * 8
    out = eng.generate([[5, 9, 33, 7]], SamplingParams(logit_bias={ref[0]: -100.0}, **base))[0]
    assert ref[0] not in out.output_ids
    # a biased request next to an unbiased one: the other row is untouched
    a, b = [eng.add_request([5, 9, 33, 7], SamplingParams(**base)),
            eng.add_request([5, 9, 33, 7], SamplingParams(logit_bias={t: 100.0}, **base))]
    while eng.has_work:
        eng.step()
    assert a.output_ids == ref and b.output_ids == [t] * 8


@pytest.mark.parametrize("async_", [False, True])
def test_min_tokens_bans_eos_and_stop_ids(model, async_):
    base = dict(max_tokens=10, temperature=0.0)
    ref = _engine(model).generate([[5, 9, 33, 7]],
                                  SamplingParams(ignore_eos=True, **base))[0].output_ids
    eos, stop = ref[1], ref[0]
    assert eos != stop

    def run(**kw):
        eng = _engine(model, async_scheduling=async_)
        eng.eos_id = eos
        s = eng.add_request([5, 9, 33, 7], SamplingParams(**base, **kw))
        while eng.has_work:
            eng.step()
        assert eng.blocks.num_free == eng.blocks.num_blocks
        return s

    assert run().output_ids == ref[:2]                       # EOS at step 2
    assert run(stop_token_ids=[stop]).output_ids == ref[:1]  # the stop id at step 1
    s = run(stop_token_ids=[stop], min_tokens=6)
    assert len(s.output_ids) >= 6
    assert eos not in s.output_ids[:5] and stop not in s.output_ids[:5]
    # from the sixth token on, EOS / the stop id end the request again
    if len(s.output_ids) < 10:
        assert s.finish_reason == "stop" and s.output_ids[-1] in (eos, stop)


def test_min_p_kept_set():
    z = torch.tensor([2.0, 1.0, 0.5, 2.0, -1.0, 2.0 + math.log(0.3) + 1e-3,
                      2.0 + math.log(0.3) - 1e-3])
    keep = min_p_keep(z, 0.3)
    assert torch.equal(keep, z >= z.max() + math.log(0.3))
    assert keep.tolist() == [True, True, False, True, False, True, False]   # 2 + ln 0.3 = 0.796
    # the same set as vLLM's probability test
    pr = torch.softmax(z.double(), -1)
    assert torch.equal(keep, pr >= 0.3 * pr.max())
    assert min_p_keep(z, 1.0).tolist() == [True, False, False, True, False, False, False]
    assert bool(min_p_keep(z, 0.0).all())


def test_process_logits_ref_matches_apply_penalties():
    g = torch.Generator().manual_seed(5)
    V, R = 97, 6
    logits = torch.randn(R, V, generator=g) * 3
    seqs = []
    for i in range(R):
        p = SamplingParams(frequency_penalty=[0.0, 0.7, -0.5][i % 3],
                           presence_penalty=[0.7, 0.0, -0.5][i % 3],
                           repetition_penalty=[1.0, 1.3][i % 2] if i else 1.3)
        s = Sequence(torch.randint(0, V, (9,), generator=g).tolist(), p)
        s.output_ids = torch.randint(0, V, (25,), generator=g).tolist()
        seqs.append(s)
    counts = torch.stack([counts_from_ids(s.prompt_ids, s.output_ids, V) for s in seqs])
    got = process_logits_ref(logits, counts, [s.params.repetition_penalty for s in seqs],
                             [s.params.frequency_penalty for s in seqs],
                             [s.params.presence_penalty for s in seqs])
    torch.testing.assert_close(got, apply_penalties(logits, seqs), rtol=1e-6, atol=1e-6)
    # a prompt id carries bit 31 only; a generated id counts
    c = counts_from_ids([3, 3, 4], [4, 4, 5], V)
    assert c[3] == 1 << 31 and c[4] == (1 << 31) + 2 and c[5] == 1 and c[6] == 0


def test_repetition_acts_on_the_biased_sign():
    """logit_bias first; the repetition penalty then sees the biased logit's sign."""
    x = torch.tensor([[1.0, 1.0, -1.0, 0.5]])
    counts = torch.tensor([[2, 2, (1 << 31), 0]])
    out = process_logits_ref(x, counts, [2.0], [1.0], [0.25],
                             bias=[([0, 3], [-3.0, -float("inf")])])
    # token 0: 1 - 3 = -2 (negative: multiplied) -> -4, then - (1.0 * 2 + 0.25) = -6.25
    assert out[0, 0].item() == -6.25
    # token 1: unbiased, positive: 1 / 2 - 2.25
    assert out[0, 1].item() == -1.75
    # token 2: in the prompt only: repetition, no frequency / presence
    assert out[0, 2].item() == -2.0
    assert out[0, 3].item() == -float("inf")
