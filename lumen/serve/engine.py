"""Serving engine: continuous batching over the paged-KV model runner.

Replaces the vLLM 0.6 engine the reference declares (README.md:10,16; requirements.txt:17-18):
``LLMEngine`` is the synchronous core (add_request / step / generate), ``AsyncEngine`` runs it
on a background thread and streams tokens to asyncio consumers (the OpenAI API server).
Adapters from training (PEFT dir) are merged into the base weights at load.
With ``tp_size > 1`` rank 0 runs this engine and ranks 1..N-1 run ``worker_loop``.
"""
from __future__ import annotations

import asyncio
import os
import queue
import threading
import time
import uuid
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Union

import numpy as np
import torch
import torch.distributed as dist

from ..models import build_model, get_config
from .block_manager import BlockManager
from .model_runner import (ModelRunner, ServeWeights, StepInput, kv_bytes_per_token,
                           process_logits_ref, sample_rows_ref)
from .sampler_state import (GuidedState, RowParams, SamplerState, advance_guided_ref, bias_csr,
                            counts_from_ids)
from .scheduler import Batch, Scheduler, SchedulerConfig
from .sequence import SamplingParams, Sequence, Status


@dataclass
class EngineConfig:
    model: str = "meta-llama/Llama-2-7b-hf"
    adapter: Optional[str] = None           # PEFT adapter dir to merge (training output)
    dtype: str = "bf16"
    max_model_len: int = 4096
    block_size: int = 16
    gpu_memory_utilization: float = 0.90
    num_blocks: Optional[int] = None
    max_num_seqs: int = 256
    # tokens per engine step (decode rows + prefill chunks): bounds the time a prefill can add
    # to a step, i.e. the inter-token latency of the running streams (chunked prefill)
    max_num_batched_tokens: int = 2048
    # x budget while at most max_num_seqs // 4 sequences decode (scheduler.SchedulerConfig).
    # Off by default: at x2 on the 256-request burst it moved TTFT p50 by -8% / +8% over two
    # runs and ITL p99 by +3-4 ms (profiles/r3d/serve_boost)
    prefill_boost: int = 1
    # "chunked": every step decodes all running streams and fills the rest of the budget with
    # prefill chunks (mixed steps: bounded inter-token latency); "prefill_first": vLLM 0.6.0's
    # default (the version the reference pins) -- prefill-only steps while prompts wait, decode
    # steps otherwise (scheduler.py)
    scheduling_policy: str = "chunked"
    tp_size: int = 1
    seed: int = 0
    use_graphs: bool = True
    device: Optional[str] = None
    init: str = "auto"
    # multi-LoRA serving (vLLM --enable-lora): {served name: PEFT adapter dir}, kept un-merged
    lora_modules: Optional[Dict[str, str]] = None
    max_loras: int = 4
    # async scheduling (TP = 1): step t+1 is scheduled, built and launched while step t runs;
    # its decode tokens come from step t's sampled tokens ON THE DEVICE, and step t's tokens
    # reach the host afterwards (EOS / stop ids are seen one step late: one wasted row)
    async_scheduling: bool = True
    # KV-cache element type: "auto" = model dtype; "fp8" = e4m3 (vLLM --kv-cache-dtype fp8):
    # twice the cache capacity and half the K/V bytes per decode step, at fp8 K/V precision
    kv_cache_dtype: str = "auto"
    # automatic prefix caching (vLLM --enable-prefix-caching): prompts share the cached K/V of
    # equal leading full blocks; finished sequences' blocks stay cached until evicted
    enable_prefix_caching: bool = False
    # weight-only quantization (vLLM --quantization): None = 16-bit weights; "fp8" = the decoder
    # projections stored as e4m3fn with one f32 scale per output row (ops/quant.py), activations
    # and accumulation unchanged; "ptpc_fp8" = the same weights with the projection inputs
    # quantized to e4m3fn per token at run time (W8A8, vLLM's ptpc_fp8 on ROCm); "mxfp4" = MXFP4
    # weights (e2m1 + one E8M0 scale per 32 k, round to nearest) with the same per-token e4m3fn
    # inputs (W4A8); "mxfp4_a16" = the same MXFP4 weights with the 16-bit activations unchanged
    # (weight-only, W4A16); embedding, norms and LM head stay 16-bit
    quantization: Optional[str] = None
    # speculative decoding by prompt lookup (vLLM --speculative-model "[ngram]"): up to this many
    # draft tokens per greedy sequence, copied from where the sequence's last n tokens (n from
    # ngram_max down to ngram_min) occurred before; a decode step then verifies every draft in
    # one forward (0 = off).  Scheduling is synchronous while it is on.
    num_speculative_tokens: int = 0
    ngram_max: int = 4
    ngram_min: int = 1
    # a verify step is a mixed forward (slower than a graph-replayed decode step): it runs only
    # when at least this fraction of the decode rows has a draft; a sequence whose drafts were
    # all rejected backs off (1, 3, 7 .. 63 steps) before it drafts again
    spec_min_fraction: float = 0.5
    # the prompt-lookup index covers the n-grams of the last ngram_window tokens of a sequence
    # (int keys, pruned as the window slides): at most ngram_window * (ngram_max - ngram_min + 1)
    # dict entries per sequence -- 4 * 1024 with the defaults, ~0.4 MB; 256 sequences ~100 MB
    ngram_window: int = 1024
    # guided decoding (lumen/serve/guided.py): a grammar may have at most this many automaton
    # states (its token table is states * V * 2 bytes: 262 MB at 4096 x 32000), and the engine
    # keeps compiled tables up to this many MB (LRU; a table in use is never evicted)
    guided_max_states: int = 4096
    guided_cache_mb: int = 1024


_DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def apply_penalties(logits: torch.Tensor, seqs: List[Sequence]) -> torch.Tensor:
    """Presence / frequency / repetition penalties on the rows of ``logits`` (f32 result), one
    scatter-add of the rows' token ids into a [rows, V] count table on the device.  Order as in
    vLLM's ``apply_penalties``: the repetition penalty first (on the raw logit's sign), then the
    frequency and presence subtractions."""
    out = logits.float().clone()
    rows = [i for i, s in enumerate(seqs) if s.params.has_penalties]
    V = out.shape[1]
    dev = out.device

    def counts(id_lists):
        L = max((len(x) for x in id_lists), default=0)
        c = torch.zeros(len(id_lists), V + 1, dtype=torch.float32, device=dev)
        if L:
            ids = torch.full((len(id_lists), L), V, dtype=torch.long)
            for j, x in enumerate(id_lists):
                if x:
                    ids[j, :len(x)] = torch.tensor(x, dtype=torch.long)
            ids = ids.to(dev)
            c.scatter_add_(1, ids, torch.ones_like(ids, dtype=torch.float32))
        return c[:, :V]

    sel = [seqs[i] for i in rows]
    ridx = torch.tensor(rows, dtype=torch.long, device=dev)
    lg = out[ridx]
    rp = torch.tensor([s.params.repetition_penalty for s in sel], device=dev)[:, None]
    if bool((rp != 1.0).any()):
        seen = (counts([s.all_ids for s in sel]) > 0) & (rp != 1.0)
        lg = torch.where(seen, torch.where(lg > 0, lg / rp, lg * rp), lg)
    out_c = counts([s.output_ids for s in sel])
    fp = torch.tensor([s.params.frequency_penalty for s in sel], device=dev)[:, None]
    pp = torch.tensor([s.params.presence_penalty for s in sel], device=dev)[:, None]
    lg = lg - (fp * out_c + pp * (out_c > 0).float())
    out[ridx] = lg
    return out


class LLMEngine:
    def __init__(self, cfg: EngineConfig, model=None, tokenizer=None):
        self.cfg = cfg
        self.tp = cfg.tp_size
        self.rank = dist.get_rank() if (self.tp > 1 and dist.is_initialized()) else 0
        if cfg.device:
            dev = torch.device(cfg.device)
        elif torch.cuda.is_available():
            dev = torch.device("cuda", torch.cuda.current_device())
        else:
            dev = torch.device("cpu")
        self.device = dev
        if dev.type == "cuda":
            from ..utils.gemm_tuning import load_tuned_gemms

            load_tuned_gemms()  # tuned hipBLASLt algorithms for the prefill/decode GEMM shapes
        dt = _DT[cfg.dtype] if dev.type == "cuda" else torch.float32
        if cfg.quantization not in (None, "fp8", "ptpc_fp8", "mxfp4", "mxfp4_a16"):
            raise ValueError("quantization must be None, 'fp8', 'ptpc_fp8', 'mxfp4' or "
                             "'mxfp4_a16', got "
                             f"{cfg.quantization}")
        own_model = model is None   # a model passed in by the caller is left untouched
        if model is None:
            model = build_model(cfg.model, dtype=dt, device=dev, init=cfg.init, seed=cfg.seed)
        if cfg.adapter:
            from ..lora import load_adapter, merge_lora

            load_adapter(model, cfg.adapter)
            merge_lora(model)
        model.eval()
        self.model_config = model.config
        tp_group = dist.group.WORLD if self.tp > 1 else None
        if self.tp > 1:
            # the host side of the step broadcast (lumen/serve/tp.py): created collectively here,
            # where every rank constructs its engine
            from ..parallel.dist import host_group

            host_group()
        # quantized after the adapter merge above; un-merged lora_modules stay 16-bit on top
        self.weights = ServeWeights(model, self.rank, self.tp, cfg.quantization,
                                    release=own_model and cfg.quantization is not None)
        if cfg.quantization is not None and dev.type == "cuda":
            torch.cuda.empty_cache()  # the released 16-bit projections become KV blocks below
        if cfg.kv_cache_dtype not in ("auto", "fp8", "mxfp4"):
            raise ValueError(f"kv_cache_dtype must be 'auto', 'fp8' or 'mxfp4', got "
                             f"{cfg.kv_cache_dtype}")
        if cfg.kv_cache_dtype == "mxfp4":
            # 4.25 bits an element: e2m1 codes + one E8M0 scale byte per 32 elements of a head row
            # (ops.attention.Mxfp4KV); round to nearest, uncalibrated
            hd = model.config.head_dim
            if hd % 32 != 0 or (cfg.block_size * hd * 17 // 32) % 4 != 0:
                raise ValueError(f"kv_cache_dtype 'mxfp4' needs head_dim % 32 == 0 (MX blocks of 32 "
                                 f"elements) and block_size * head_dim * 17 / 32 a multiple of 4 "
                                 f"bytes; this model has head_dim {hd}, block_size {cfg.block_size}")
            self.kv_dtype = "mxfp4"
        else:
            self.kv_dtype = torch.float8_e4m3fn if cfg.kv_cache_dtype == "fp8" else dt
        nb = cfg.num_blocks or self._auto_blocks(self.kv_dtype)
        if self.tp > 1 and dist.is_initialized():
            # one block count for the whole TP group: rank 0 schedules block ids that every
            # worker's cache must hold (free memory, hence the auto count, can differ per rank)
            from ..parallel.dist import host_group

            t = torch.tensor([nb], dtype=torch.int64)
            dist.all_reduce(t, op=dist.ReduceOp.MIN, group=host_group())
            nb = int(t.item())
        self.blocks = BlockManager(nb, cfg.block_size, prefix_caching=cfg.enable_prefix_caching)
        car = None
        if self.tp > 1 and dev.type == "cuda":
            # TP decode: row-parallel sums on the custom IPC all-reduce, which also lets the
            # decode buckets be captured in hipGraphs (collective: every rank builds it here)
            from ..parallel.custom_ar import maybe_custom_allreduce

            esz = torch.empty((), dtype=dt).element_size()
            rows = min(256, cfg.max_num_seqs)
            vshard = model.config.vocab_size // self.tp
            car = maybe_custom_allreduce(
                tp_group, dev, max(8 << 20, rows * model.config.hidden_size * esz,
                                   rows * vshard * esz))
        self.runner = ModelRunner(self.weights, nb, cfg.block_size, dev, cfg.max_model_len,
                                  tp_group, use_graphs=cfg.use_graphs,
                                  max_graph_batch=min(256, cfg.max_num_seqs), custom_ar=car,
                                  kv_dtype=self.kv_dtype)
        self.lora_names: List[str] = []
        if cfg.lora_modules:
            from .multi_lora import MultiLoRA

            self.runner.lora = MultiLoRA(model.config, cfg.lora_modules, cfg.max_loras, self.rank,
                                         self.tp, dev, dt)
            self.lora_names = list(self.runner.lora.names)
        self._pinned: List[Optional[torch.Tensor]] = [None, None]
        self._pinned_ready: List[Optional[object]] = [None, None]
        self._pin_i = 0
        # TP > 1 too: a step is broadcast when it is launched, its decode tokens straight from
        # the device (gathered from the previous step's samples), so workers never wait for
        # rank 0's host to see the tokens
        self.spec_k = max(0, int(cfg.num_speculative_tokens))
        # drafting reads every sequence's latest token on the host: no step in flight
        self.async_sched = bool(cfg.async_scheduling) and self.spec_k == 0
        self._inflight: Optional[dict] = None
        self.scheduler = Scheduler(SchedulerConfig(
            cfg.max_num_seqs, cfg.max_num_batched_tokens, cfg.max_model_len,
            prefill_boost=max(1, int(cfg.prefill_boost)), policy=cfg.scheduling_policy),
            self.blocks)
        if tokenizer is None:
            from ..data.tokenizer import load_tokenizer

            tokenizer = load_tokenizer(cfg.model, self.model_config.vocab_size)
        self.tokenizer = tokenizer
        self.eos_id = getattr(tokenizer, "eos_token_id", self.model_config.eos_token_id)
        self.step_count = 0
        # penalty counts of the running sequences on the device (allocated at the first request
        # with a penalty); LUMEN_SAMPLER_STATE=0 forces the host path (apply_penalties) for A/B
        # runs.  Rank 0 only: TP workers never sample.
        from ..ops._native import native
        self.dev_state = (dev.type == "cuda" and native() is not None
                          and os.environ.get("LUMEN_DISABLE_NATIVE", "0") != "1"
                          and os.environ.get("LUMEN_SAMPLER_STATE", "1") != "0")
        self.sampler_state = SamplerState(cfg.max_num_seqs, self.model_config.vocab_size, dev)
        # guided decoding: the automaton state of the running guided sequences, next to the
        # counts; token tables are compiled per grammar and cached (guided.GuidedCache)
        from .guided import GuidedCache
        self.guided_state = GuidedState(cfg.max_num_seqs, dev)
        self.guided_cache = GuidedCache(int(cfg.guided_cache_mb) << 20)
        self._token_bytes = None
        self.guided_requests = 0

        def on_release(seq):
            self.sampler_state.release(seq)
            self.guided_state.release(seq)
            if seq.finished:
                self.guided_cache.evict()
        self.scheduler.on_release = on_release
        self.stats = {"prefill_tokens": 0, "decode_tokens": 0, "steps": 0, "requests": 0,
                      "finished": 0, "overlapped_steps": 0, "spec_proposed": 0,
                      "spec_accepted": 0, "spec_steps": 0}

    # --------------------------------------------------------------------------------------
    def _auto_blocks(self, dt) -> int:
        esz = 17 / 32 if dt == "mxfp4" else torch.tensor([], dtype=dt).element_size()
        per_tok = kv_bytes_per_token(self.model_config, esz, self.tp)
        per_block = per_tok * self.cfg.block_size
        if self.device.type == "cuda":
            free, total = torch.cuda.mem_get_info(self.device)
            budget = free - (1 - self.cfg.gpu_memory_utilization) * total
            budget -= 4 << 30  # activations / graphs / workspace headroom
            if os.environ.get("LUMEN_SHARED_GPU_REHEARSAL") == "1" and self.tp > 1:
                # ranks sharing one device (rehearsal) each see the same free memory before any
                # of them allocates: split it, or the last rank to allocate runs out
                budget /= self.tp
        else:
            budget = 256 << 20
        nb = int(max(budget, per_block * 64) // per_block)
        cap = self.cfg.max_num_seqs * ((self.cfg.max_model_len + self.cfg.block_size - 1)
                                       // self.cfg.block_size) + 64
        return max(64, min(nb, cap))

    def encode(self, prompt: Union[str, List[int]]) -> List[int]:
        if isinstance(prompt, str):
            return self.tokenizer.encode(prompt)
        return list(prompt)

    def add_request(self, prompt: Union[str, List[int]], params: Optional[SamplingParams] = None,
                    request_id: Optional[str] = None, lora: Optional[str] = None) -> Sequence:
        params = params or SamplingParams()
        ids = self.encode(prompt)
        if not ids:
            raise ValueError("empty prompt")
        budget = self.cfg.max_model_len - len(ids)
        if budget < 1:
            raise ValueError(f"prompt ({len(ids)} tokens) does not fit max_model_len "
                             f"{self.cfg.max_model_len}")
        if params.max_tokens > budget:
            params.max_tokens = budget
        if params.prompt_logprobs is not None and self.tp > 1:
            raise ValueError("prompt_logprobs is served at tensor-parallel size 1 only")
        if params.min_tokens > params.max_tokens:
            params.min_tokens = params.max_tokens
        if params.logit_bias:
            V = self.model_config.vocab_size
            bad = [t for t in params.logit_bias if not 0 <= t < V]
            if bad:
                raise ValueError(f"logit_bias token id {bad[0]} is outside the vocabulary "
                                 f"(0..{V - 1})")
        table = self._guided_table(params) if params.guided is not None else None
        seq = Sequence(ids, params, request_id or uuid.uuid4().hex)
        if table is not None:
            seq.guided_table = table
            table.refs += 1
            self.guided_requests += 1
        if lora:
            if self.runner.lora is None or lora not in self.lora_names:
                raise ValueError(f"unknown LoRA adapter '{lora}' (serving: {self.lora_names})")
            seq.lora_slot = self.runner.lora.slot_of(lora)
        self.scheduler.add(seq)
        self.stats["requests"] += 1
        return seq

    def token_bytes(self):
        if self._token_bytes is None:
            from .guided import token_bytes
            self._token_bytes = token_bytes(self.tokenizer)
        return self._token_bytes

    def _guided_table(self, params: SamplingParams):
        """The token table of the request's grammar, from the cache or built now (on the
        engine's device).  ``ValueError`` for what the compiler rejects."""
        from .guided import (Grammar, TokenTable, build_token_index, compile_guided,
                             guided_digest, tokenizer_identity)

        kind, payload = params.guided
        if self.eos_id is None:
            raise ValueError("guided decoding needs a tokenizer with an EOS token")
        key = guided_digest(kind, payload) + "|" + tokenizer_identity(self.tokenizer)
        cap = int(self.cfg.guided_max_states)

        def build():
            if params.guided_dfa is not None:
                trans, accept = params.guided_dfa
                g = Grammar(kind, payload, np.asarray(trans, dtype=np.int32),
                            np.asarray(accept, dtype=bool))
            else:
                g = compile_guided(kind, payload, cap)
            if g.num_states > cap:
                raise ValueError(f"grammar needs {g.num_states} states, more than the limit of "
                                 f"{cap} (--guided-max-states)")
            nxt, live = build_token_index(g.trans, g.accept, self.token_bytes(),
                                          self.model_config.vocab_size, self.eos_id, self.device)
            return TokenTable(g, nxt, live)

        table = self.guided_cache.get(key, build)
        params.guided_dfa = None     # the table holds the grammar; requests need not carry it
        return table

    def guided_stats(self) -> dict:
        c = self.guided_cache
        return {"guided_requests": self.guided_requests, "guided_cache_hits": c.hits,
                "guided_compile_seconds": c.compile_seconds, "guided_cache_bytes": c.nbytes}

    def _guided_resume_state(self, s: Sequence) -> int:
        """The automaton state of a sequence that is sampled for the first time or again after a
        preemption: its host output ids walked through the grammar with the token bytes."""
        if not s.output_ids:
            return 0
        g = s.guided_table.grammar
        tb = self.token_bytes()
        st = 0
        for t in s.output_ids:
            b = tb[t] if 0 <= t < len(tb) else None
            if b is None:
                continue             # EOS / a special token leaves the state alone
            n = g.walk(b, st)
            if n >= 0:
                st = n
        return st

    def abort(self, request_id: str) -> None:
        self.scheduler.abort(request_id)

    @property
    def has_work(self) -> bool:
        return self.scheduler.has_work or self._inflight is not None

    # --------------------------------------------------------------------------------------
    def _build_input(self, batch: Batch) -> StepInput:
        """Host-side step metadata, vectorised with numpy and shipped in ONE host-to-device copy
        (a Python/torch loop per sequence cost ~10 ms per 256-sequence decode step, a third of
        the step).  Rows: prefill chunks first, then decode tokens."""
        bm = self.blocks
        bs = bm.block_size
        use_lora = self.runner.lora is not None
        toks, pos, slots, lora = [], [], [], []
        cu, kv_lens, ptables = [0], [], []
        for s, c in batch.prefills:
            a = s.num_cached
            ids = s.all_ids + s.draft if s.draft else s.all_ids
            toks.append(np.asarray(ids[a:a + c], dtype=np.int64))
            p = np.arange(a, a + c, dtype=np.int64)
            pos.append(p)
            tbl = np.asarray(bm.tables[s.seq_id], dtype=np.int64)
            slots.append(tbl[p // bs] * bs + p % bs)
            cu.append(cu[-1] + c)
            kv_lens.append(a + c)
            ptables.append(tbl)
            if use_lora:
                lora.append(np.full(c, s.lora_slot, dtype=np.int64))
        # prompt_logprobs: the row at position p scores prompt token p + 1
        prows: List[int] = []
        pmeta = []
        for i, (s, c) in enumerate(batch.prefills):
            if s.params.prompt_logprobs is None:
                continue
            a = s.num_cached
            hi = min(a + c, len(s.prompt_ids) - 1)
            if hi > a:
                pmeta.append((s, a + 1, hi - a, len(prows)))
                prows.extend(range(cu[i], cu[i] + hi - a))
        Tp = cu[-1]
        N = len(batch.decodes)
        parts = toks + pos + slots
        dec_bt = None
        maxb_d = 0
        if N:
            tables = [bm.tables[s.seq_id] for s in batch.decodes]
            lens = np.fromiter((s.length for s in batch.decodes), dtype=np.int64, count=N)
            dtok = np.fromiter((s.last_token for s in batch.decodes), dtype=np.int64, count=N)
            maxb_d = max(len(t) for t in tables)
            dec_bt = np.zeros((N, maxb_d), dtype=np.int64)
            for i, t in enumerate(tables):
                dec_bt[i, :len(t)] = t
            dpos = lens - 1
            dslots = dec_bt[np.arange(N), dpos // bs] * bs + dpos % bs
            # decode rows go after the prefill rows in each of tokens / positions / slots
            parts = toks + [dtok] + pos + [dpos] + slots + [dslots]
            if use_lora:
                lora.append(np.fromiter((s.lora_slot for s in batch.decodes), dtype=np.int64,
                                        count=N))
        T = Tp + N
        P = len(batch.prefills)
        maxb_p = max((len(t) for t in ptables), default=0)
        extra = []
        if P:
            pt = np.zeros((P, maxb_p), dtype=np.int64)
            for i, t in enumerate(ptables):
                pt[i, :len(t)] = t
            extra += [pt.reshape(-1), np.asarray(kv_lens, dtype=np.int64)]
        if N:
            extra += [dec_bt.reshape(-1), lens]
        src = None
        if N and self._inflight is not None:
            # decode inputs still being sampled by the in-flight step: row of its token tensor
            row = self._inflight["row"]
            src = np.fromiter((row.get(s.seq_id, -1) if s.has_pending else -1
                               for s in batch.decodes), dtype=np.int64, count=N)
            if not (src >= 0).any():
                src = None
            else:
                extra.append(src)
        if batch.kind == "verify":
            # speculative verification: every row of a drafted chunk is scored
            done_rows = list(range(Tp))
            rseqs = [s for s, c in batch.prefills for _ in range(c)] + batch.decodes
            ps = [s.params for s in rseqs]
        else:
            n_done = len(batch.completing())
            done_rows = [cu[i + 1] - 1 for i, (s, c) in enumerate(batch.prefills)
                         if s.num_cached + c == s.length]
            assert len(done_rows) == n_done
            rseqs = batch.sampled
            ps = [s.params for s in rseqs]
        rows = np.concatenate([np.asarray(done_rows, dtype=np.int64),
                               np.arange(Tp, T, dtype=np.int64)])
        extra.append(rows)
        R = len(rows)
        if R:
            # sampling parameters of the sampled rows ride in the same async copy: building them
            # with torch.tensor(list, device=...) is a blocking copy -- a stream synchronise per
            # step that would serialise the host with the GPU and undo async scheduling
            extra += [np.fromiter((p.temperature for p in ps), np.float64, R).view(np.int64),
                      np.fromiter((p.top_p for p in ps), np.float64, R).view(np.int64),
                      np.fromiter((p.top_k for p in ps), np.int64, R)]
        rowp = None
        if R and any(p.row_features or (self.dev_state and p.has_penalties) for p in ps):
            rowp = self._row_params(batch, rseqs, ps, Tp)
            extra += rowp["pack"]
        if prows:
            extra.append(np.asarray(prows, dtype=np.int64))
        if use_lora:
            extra.append(np.concatenate(lora))
        host = np.concatenate([np.concatenate(parts)] + extra)
        dev = self._to_device(host)
        o = 3 * T
        inp = StepInput("mixed" if batch.kind == "verify" else batch.kind, dev[:T],
                        dev[T:2 * T].int(), dev[2 * T:3 * T], cu)
        if P:
            inp.prefill_tables = dev[o:o + P * maxb_p].view(P, maxb_p).int()
            o += P * maxb_p
            inp.kv_lens = kv_lens
            inp.kv_lens_t = dev[o:o + P].int()
            o += P
        if N:
            inp.block_tables = dev[o:o + N * maxb_d].view(N, maxb_d).int()
            o += N * maxb_d
            inp.context_lens = dev[o:o + N].int()
            o += N
            inp.max_context = int(lens.max())
        if src is not None:
            # dependent decode tokens: gathered from the previous step's sampled tokens here,
            # on the stream, before the step reads (or its graph copies in) its token row
            s_dev = dev[o:o + N]
            o += N
            prev = self._inflight["toks"]
            inp.tokens[Tp:] = torch.where(s_dev >= 0, prev[s_dev.clamp(min=0)], inp.tokens[Tp:])
        inp.sample_rows = dev[o:o + R]
        o += R
        if R:
            inp.temps = dev[o:o + R].view(torch.float64).float()
            inp.top_ps = dev[o + R:o + 2 * R].view(torch.float64).float()
            inp.top_ks = dev[o + 2 * R:o + 3 * R].int()
            o += 3 * R
        if rowp is not None:
            o = self._unpack_row_params(inp, rowp, dev, o, R)
        if prows:
            inp.extra_rows = dev[o:o + len(prows)]
            inp.prompt_meta = pmeta
            o += len(prows)
        if use_lora:
            inp.lora_ids = dev[o:o + T].int()
        return inp

    def _row_bias(self, s: Sequence, k: int = 0):
        """(ids, values) of the row's logit_bias entries, with min_tokens lowered to -inf entries
        for EOS and the stop ids while the sequence (its in-flight tokens and ``k`` more
        counted) is below min_tokens; None when it has neither."""
        p = s.params
        ban = p.min_tokens > 0 and s.num_generated + k < p.min_tokens
        if p.logit_bias is None and not ban:
            return None
        if not ban:
            if s.bias_np is None:
                s.bias_np = (np.fromiter(p.logit_bias.keys(), np.int64, len(p.logit_bias)),
                             np.fromiter(p.logit_bias.values(), np.float64, len(p.logit_bias)))
            return s.bias_np
        V = self.model_config.vocab_size
        d = dict(p.logit_bias or {})
        stops = list(p.stop_token_ids)
        if not p.ignore_eos and self.eos_id is not None:
            stops.append(self.eos_id)
        for t in stops:
            if 0 <= t < V:
                d[int(t)] = -float("inf")
        return (np.fromiter(d.keys(), np.int64, len(d)), np.fromiter(d.values(), np.float64, len(d)))

    def _row_params(self, batch: Batch, rseqs: List[Sequence], ps, Tp: int) -> dict:
        """Host arrays of the per-row sampler arguments of this step (they ride in the packed
        step copy), and the state slots of the sequences that are sampled for the first time.
        A request with a seed draws from (its seed, tokens generated so far, 0): the same
        tokens whatever else runs; one without from (engine seed, step, its row)."""
        R = len(rseqs)
        verify = batch.kind == "verify"
        # rows of a drafted chunk (verify steps): greedy, no bias, no state -- _propose drafts
        # only such sequences; k = the row's position in its chunk
        kpos = np.zeros(R, dtype=np.int64)
        if verify and Tp:
            kpos[:Tp] = np.concatenate([np.arange(c) for _, c in batch.prefills])
        eseed = int(self.cfg.seed) & 0x7FFFFFFFFFFFFFFF
        seeded = np.fromiter((p.seed is not None for p in ps), np.bool_, R)
        seed = np.fromiter((eseed if p.seed is None else int(p.seed) & 0x7FFFFFFFFFFFFFFF
                            for p in ps), np.int64, R)
        gen = np.fromiter((s.num_generated for s in rseqs), np.int64, R) + kpos
        offset = np.where(seeded, gen, self.step_count)
        rngrow = np.where(seeded, 0, np.arange(R, dtype=np.int64))
        new = []
        if self.dev_state:
            st = self.sampler_state
            for i, s in enumerate(rseqs):
                if ps[i].has_penalties and s.state_slot < 0 and not (verify and i < Tp):
                    s.state_slot = st.acquire()
                    new.append(s)
        slot = np.fromiter((-1 if (verify and i < Tp) else s.state_slot
                            for i, s in enumerate(rseqs)), np.int64, R)
        # guided rows: the table's address and the sequence's automaton-state slot (verify rows
        # of a drafted chunk carry none: _propose drafts no guided sequence)
        gnew = []
        guided = any(s.guided_table is not None for s in rseqs)
        if guided:
            gs = self.guided_state
            for i, s in enumerate(rseqs):
                if s.guided_table is not None and s.guided_slot < 0 and not (verify and i < Tp):
                    s.guided_slot = gs.acquire()
                    gnew.append(s)
            grow = [s.guided_table is not None and not (verify and i < Tp)
                    for i, s in enumerate(rseqs)]
            gaddr = np.fromiter((s.guided_table.address if g else 0
                                 for g, s in zip(grow, rseqs)), np.int64, R)
            gslot = np.fromiter((s.guided_slot if g else -1 for g, s in zip(grow, rseqs)),
                                np.int64, R)
        f4 = np.concatenate([np.fromiter((p.min_p for p in ps), np.float64, R),
                             np.fromiter((p.repetition_penalty for p in ps), np.float64, R),
                             np.fromiter((p.frequency_penalty for p in ps), np.float64, R),
                             np.fromiter((p.presence_penalty for p in ps), np.float64, R)])
        bias = [None if (verify and i < Tp) or not (ps[i].logit_bias or ps[i].min_tokens)
                else self._row_bias(s, int(kpos[i])) for i, s in enumerate(rseqs)]
        bptr, bidx, bval = bias_csr(bias)
        nb = len(bidx)
        pack = [seed, offset, rngrow, f4.view(np.int64), slot]
        if nb:
            pack += [bptr, bidx, bval.view(np.int64)]
        if guided:
            pack += [gaddr, gslot,
                     np.fromiter((s.guided_slot for s in gnew), np.int64, len(gnew)),
                     np.fromiter((self._guided_resume_state(s) for s in gnew), np.int64,
                                 len(gnew))]
        n_ids = 0
        if new:
            lens = np.fromiter((len(s.prompt_ids) + len(s.output_ids) for s in new), np.int64,
                               len(new))
            iptr = np.zeros(len(new) + 1, dtype=np.int64)
            np.cumsum(lens, out=iptr[1:])
            n_ids = int(iptr[-1])
            pack += [np.fromiter((s.state_slot for s in new), np.int64, len(new)), iptr,
                     np.fromiter((len(s.prompt_ids) for s in new), np.int64, len(new))]
            pack += [np.asarray(s.prompt_ids + s.output_ids, dtype=np.int64) for s in new]
        host = {"seeds": [p.seed for p in ps], "offsets": offset, "bias": bias, "seqs": rseqs,
                "min_p": f4[:R], "rp": f4[R:2 * R], "fp": f4[2 * R:3 * R], "pp": f4[3 * R:]}
        if guided:
            host["g_tables"] = [s.guided_table.next if g else None for g, s in zip(grow, rseqs)]
            host["g_slots"] = gslot
        return {"pack": pack, "nb": nb, "new": len(new), "n_ids": n_ids, "host": host,
                "guided": guided, "gnew": len(gnew)}

    @staticmethod
    def _unpack_row_params(inp: StepInput, rowp: dict, dev: torch.Tensor, o: int, R: int) -> int:
        """The device views of ``_row_params``'s arrays in the packed copy ``dev`` from ``o``."""
        seed, offset, rngrow = dev[o:o + R], dev[o + R:o + 2 * R], dev[o + 2 * R:o + 3 * R]
        o += 3 * R
        f4 = dev[o:o + 4 * R].view(torch.float64).float()
        o += 4 * R
        nb, n, n_ids = rowp["nb"], rowp["new"], rowp["n_ids"]
        ni = R + ((R + 1 + nb) if nb else 0)
        ints = dev[o:o + ni].int()    # slot | bias_ptr | bias_idx in one conversion
        o += ni
        sp = RowParams(seed, offset, rngrow, f4[:R], ints[:R], f4[R:2 * R], f4[2 * R:3 * R],
                       f4[3 * R:], host=rowp["host"])
        if nb:
            sp.bias_ptr, sp.bias_idx = ints[R:2 * R + 1], ints[2 * R + 1:]
            sp.bias_val = dev[o:o + nb].view(torch.float64).float()
            o += nb
        if rowp["guided"]:
            gn = rowp["gnew"]
            sp.g_table, sp.g_slot = dev[o:o + R], dev[o + R:o + 2 * R].int()
            o += 2 * R
            if gn:
                sp.host["g_init"] = (dev[o:o + gn], dev[o + gn:o + 2 * gn].int())
                o += 2 * gn
        if n:
            init = dev[o:o + 3 * n + 1 + n_ids].int()
            o += 3 * n + 1 + n_ids
            sp.host["init"] = (init[:n], init[n:2 * n + 1], init[2 * n + 1:3 * n + 1],
                               init[3 * n + 1:])
        inp.samp = sp
        return o

    def _sample(self, inp: StepInput, logits: torch.Tensor, rseqs: List[Sequence],
                want_x: bool = False):
        """Sample the step's rows (``rseqs``: the sequence of each row).  Returns (tokens,
        logprobs, the logits the tokens were drawn from).  Steps that use no per-request seed,
        min_p, logit_bias, min_tokens or device-side penalty take the plain ``sample`` entry
        with today's arguments; the others the per-row entry (kernels/sampling_rows.hip), or
        the torch references where there is no native extension."""
        ps = [s.params for s in rseqs]
        sp = inp.samp
        host_pen = not self.dev_state and any(p.has_penalties for p in ps)
        if sp is None:
            if host_pen:
                logits = apply_penalties(logits, rseqs)
            seed = self.cfg.seed if ps[0].seed is None else ps[0].seed
            t, lp = self.runner.sample(logits, inp.temps, inp.top_ps, inp.top_ks, seed,
                                       self.step_count, want_logprobs=True)
            return t, lp, logits
        h = sp.host
        gstate = None
        if sp.g_table is not None:
            # newly admitted guided sequences: their automaton state, before this step's launch
            if "g_init" in h:
                self.guided_state.write(*h.pop("g_init"))
            gstate = self.guided_state.state
        if not (logits.is_cuda and self._native_rows(logits)):
            counts = None
            if host_pen:
                V = logits.shape[1]
                counts = torch.stack([
                    counts_from_ids(s.prompt_ids, s.output_ids, V) if s.params.has_penalties
                    else torch.zeros(V, dtype=torch.int64) for s in rseqs])
            mask = None
            if gstate is not None:
                mask = [None if nx is None else nx[int(gstate[int(h["g_slots"][i])])] < 0
                        for i, nx in enumerate(h["g_tables"])]
            x = process_logits_ref(logits, counts, h["rp"], h["fp"], h["pp"], bias=h["bias"],
                                   mask=mask)
            t, lp = sample_rows_ref(x, inp.temps, inp.top_ps, inp.top_ks, h["min_p"],
                                    h["seeds"], h["offsets"], self.cfg.seed, self.step_count)
            if gstate is not None:
                advance_guided_ref(gstate, h["g_tables"], h["g_slots"], t)
            return t, lp, x
        counts = None
        if "init" in h:
            self.sampler_state.init_slots(*h.pop("init"))
        if self.dev_state and self.sampler_state.allocated:
            counts = self.sampler_state.counts
        pre = False
        if host_pen:
            # LUMEN_SAMPLER_STATE=0: the bias on the device, then the host-side penalties
            logits = apply_penalties(self.runner.logits_process(logits, sp, gstate=gstate), rseqs)
            pre = True
        elif want_x:
            logits = self.runner.logits_process(logits, sp, counts, gstate=gstate)
            pre = True
        t, lp = self.runner.sample_rows(logits, inp.temps, inp.top_ps, inp.top_ks, sp, counts,
                                        pre=pre, want_logprobs=True, gstate=gstate)
        return t, lp, logits

    @staticmethod
    def _native_rows(logits: torch.Tensor) -> bool:
        from ..ops._native import use_native
        return use_native(logits)

    def _to_device(self, host: "np.ndarray") -> torch.Tensor:
        t = torch.from_numpy(host)
        if self.device.type != "cuda":
            return t
        # two pinned staging buffers, alternating: the copy of step t-1 (queued behind step t-2's
        # kernels) never makes the host wait while it builds step t
        i = self._pin_i
        self._pin_i ^= 1
        if self._pinned_ready[i] is not None:
            self._pinned_ready[i].synchronize()  # that buffer's last copy has been read
        if self._pinned[i] is None or self._pinned[i].numel() < t.numel():
            self._pinned[i] = torch.empty(max(t.numel(), 1 << 16), dtype=torch.long).pin_memory()
        buf = self._pinned[i][:t.numel()]
        buf.copy_(t)
        out = buf.to(self.device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._pinned_ready[i] = ev
        return out

    def _broadcast(self, inp: Optional[StepInput]):
        """TP: ship the step to worker ranks as two int64 tensors (header + payload)."""
        from .tp import pack_step

        pack_step(inp, self.device)

    def step(self) -> List[Sequence]:
        """Run one engine iteration; returns sequences that received a token this step."""
        if not self.async_sched:
            batch = self.scheduler.schedule()
            if batch is None:
                return []
            if self.spec_k and batch.kind == "decode" and self._propose(batch):
                return self._run_verify(batch)
            return self._run_batch(batch)
        batch = self.scheduler.schedule()
        if batch is None:
            return self._resolve()
        if any(s.params.wants_extras for s in batch.seqs):
            # logprob alternatives / prompt scores: this step runs resolved (synchronously)
            done = self._resolve() if self._inflight is not None else []
            batch = self._drop_finished(batch)
            return done + (self._run_batch(batch) if batch is not None else [])
        if self._inflight is not None and self._needs_host_tokens(batch):
            done = self._resolve()     # this step reads real token values on the host
            # the resolved tokens may have finished (EOS / stop id / max_tokens) sequences of
            # the batch just built: their KV tables are freed, so they must not run again
            batch = self._drop_finished(batch)
            if batch is not None:
                self._launch(batch)
            return done
        prev = self._inflight
        self._launch(batch)            # step t+1 is queued behind step t ...
        if prev is None:               # (nothing older in flight: t+1 stays in flight)
            return []
        self.stats["overlapped_steps"] += 1
        return self._resolve(prev)     # ... while the host collects step t's tokens

    @staticmethod
    def _drop_finished(batch: Batch) -> Optional[Batch]:
        """The batch without the sequences that finished after it was scheduled (None if
        nothing is left).  A finished prefill's chunk and a finished decode's row just vanish:
        their blocks were already returned by ``finish_seqs``."""
        pre = [(s, c) for s, c in batch.prefills if not s.finished]
        dec = [s for s in batch.decodes if not s.finished]
        if not pre and not dec:
            return None
        return Batch("mixed" if pre else "decode", pre, dec)

    def _needs_host_tokens(self, batch: Batch) -> bool:
        """Prefill rows re-reading generated tokens (preemption recompute) need the in-flight
        step's token VALUES on the host; so do penalties on the host path (no native extension,
        or LUMEN_SAMPLER_STATE=0) -- with the device state the sampler keeps the counts."""
        return (any(s.has_pending for s, _ in batch.prefills)
                or (not self.dev_state
                    and any(s.params.has_penalties for s in batch.sampled)))

    def _launch(self, batch: Batch) -> None:
        inp = self._build_input(batch)
        if self.tp > 1:
            self._broadcast(inp)
        sampled = batch.sampled
        if batch.kind == "decode":
            logits = self.runner.decode(inp)
        else:
            logits = self.runner.execute(inp)
        self.stats["prefill_tokens"] += inp.num_prefill_rows
        self.stats["decode_tokens"] += len(batch.decodes)
        rec = {"sampled": [], "row": {}, "toks": None}
        if sampled:
            t, lp, _ = self._sample(inp, logits, sampled)
            R = t.shape[0]
            th = torch.empty(R, dtype=torch.long, pin_memory=self.device.type == "cuda")
            th.copy_(t, non_blocking=True)
            lh = None
            if lp is not None:
                lh = torch.empty(R, dtype=torch.float32, pin_memory=self.device.type == "cuda")
                lh.copy_(lp, non_blocking=True)
            ev = torch.cuda.Event() if self.device.type == "cuda" else None
            if ev is not None:
                ev.record()
            rec.update(toks=t, th=th, lh=lh, ev=ev, sampled=sampled)
        self.scheduler.launched(batch)
        for s, c in batch.prefills:
            s.num_cached += c
        for s in batch.decodes:
            s.num_cached = s.length
        for i, s in enumerate(sampled):
            s.prefilled = True
            rec["row"][s.seq_id] = i
            s.reserve()
        self.stats["steps"] += 1
        self.step_count += 1
        self._inflight = rec if sampled else None

    def _resolve(self, rec: Optional[dict] = None) -> List[Sequence]:
        """Bring a launched step's sampled tokens to the host and apply them."""
        if rec is None:
            rec, self._inflight = self._inflight, None
        if rec is None or not rec["sampled"]:
            return []
        if rec["ev"] is not None:
            rec["ev"].synchronize()
        toks = rec["th"].tolist()
        lps = rec["lh"].tolist() if rec["lh"] is not None else [None] * len(toks)
        nxt = self._inflight if self._inflight is not rec else None
        out, ended = [], []
        for s in rec["sampled"]:
            i = rec["row"].get(s.seq_id)
            if i is None:
                continue
            if s.finished:            # aborted while in flight
                s.n_pending = 0
                continue
            s.fill(int(toks[i]), lps[i], self.eos_id)
            if s.finished:
                ended.append(s)
                if nxt is not None and nxt["row"].pop(s.seq_id, None) is not None:
                    # EOS / stop id seen one step late: the next step's row for it is wasted
                    s.n_pending -= 1
            out.append(s)
        self.runner.check_collectives()
        self.stats["finished"] += len(self.scheduler.finish_seqs(ended))
        return out

    def _run_batch(self, batch: Batch) -> List[Sequence]:
        inp = self._build_input(batch)
        if self.tp > 1:
            self._broadcast(inp)
        sampled = batch.sampled   # before the cache bookkeeping below changes num_cached
        if batch.kind == "decode":
            logits = self.runner.decode(inp)
        else:
            logits = self.runner.execute(inp)
        self.stats["prefill_tokens"] += inp.num_prefill_rows
        self.stats["decode_tokens"] += len(batch.decodes)
        toks, lps = [], []
        if sampled:
            # alternatives (_extras) are read from the processed logits the token is drawn from
            t, lp, logits = self._sample(inp, logits, sampled,
                                         want_x=any(s.params.top_logprobs for s in sampled))
            toks = t.tolist()
            lps = lp.tolist() if lp is not None else [None] * len(toks)
        tops = self._extras(inp, logits, sampled)
        self.runner.check_collectives()  # a timed-out TP reduction never returns its tokens
        self.scheduler.launched(batch)
        for s, c in batch.prefills:
            s.num_cached += c
        for s in batch.decodes:
            s.num_cached = s.length
        for s, t, lp, top in zip(sampled, toks, lps, tops):
            s.prefilled = True
            s.append(int(t), lp, self.eos_id, top)
        done = self.scheduler.finish(batch)
        self.stats["finished"] += len(done)
        self.stats["steps"] += 1
        self.step_count += 1
        return sampled

    # ---- speculative decoding (prompt lookup) ----------------------------------------------
    @staticmethod
    def _ngram_key(ids: List[int], a: int, b: int) -> int:
        return hash(tuple(ids[a:b]))

    def _lookup(self, ids: List[int], k: int, s: Optional[Sequence] = None) -> List[int]:
        """Up to k tokens that followed the most recent earlier occurrence of the sequence's
        last n tokens (n = ngram_max .. ngram_min) within its last ``ngram_window`` tokens.
        The n-gram index of ``s`` (int hash of the n-gram -> position after it) is extended
        incrementally -- a few dict updates per new token, where a scan of the history cost
        ~60 us per sequence, 15 ms per 256-row step -- and pruned as the window slides, so its
        size is bounded.  A hash collision can only propose a wrong draft, which the verify
        step rejects (outputs stay identical to plain decoding)."""
        lo, hi = max(1, self.cfg.ngram_min), self.cfg.ngram_max
        W = max(1, int(self.cfg.ngram_window))
        idx = s.ngram_idx if s is not None else {}
        upto = s.ngram_upto if s is not None else 0
        L = len(ids)
        start = max(upto, L - 1 - W)
        key = self._ngram_key
        for p in range(start, L - 1):          # n-grams ending before the current suffix
            for n in range(lo, min(hi, p + 1) + 1):
                idx[key(ids, p - n + 1, p + 1)] = p + 1
        if s is not None:
            # n-grams ending before the window start leave the index (unless a later
            # occurrence has taken the key over)
            for p in range(max(0, upto - W - 1), max(0, L - 1 - W)):
                for n in range(lo, min(hi, p + 1) + 1):
                    kk = key(ids, p - n + 1, p + 1)
                    if idx.get(kk) == p + 1:
                        del idx[kk]
            s.ngram_upto = max(upto, L - 1)
        for n in range(min(hi, L - 1), lo - 1, -1):
            j = idx.get(key(ids, L - n, L))
            if j is not None and j < L:
                return ids[j:j + k]
        return []

    def _propose(self, batch: Batch) -> bool:
        """Drafts for the greedy decode rows of ``batch`` (``Sequence.draft``), their KV slots
        reserved; False when nothing was drafted.  The spec_min_fraction check and the token
        budget (verify rows + plain decode rows <= max_num_batched_tokens) are applied BEFORE
        any block is reserved, so dropped drafts never grow a table or evict cached blocks."""
        if any(s.params.wants_extras for s in batch.decodes):
            return False                      # alternatives are computed on the plain path
        cand = []
        for s in batch.decodes:
            p = s.params
            if p.temperature > 0 or p.has_penalties or p.wants_extras:
                continue
            if p.logit_bias or s.num_generated < p.min_tokens or p.guided is not None:
                continue                      # drafted rows carry no bias, no bans and no mask
            if s.spec_wait > 0:
                s.spec_wait -= 1
                continue
            room = min(self.spec_k, p.max_tokens - len(s.output_ids) - 1,
                       self.cfg.max_model_len - s.length - 1)
            if room <= 0:
                continue
            d = self._lookup(s.all_ids, room, s)
            if d:
                cand.append((s, d))
        # budget: every decode row costs 1, a draft adds len(d) verify rows
        spare = self.cfg.max_num_batched_tokens - len(batch.decodes)
        kept = []
        for s, d in cand:
            d = d[:max(0, spare)]
            if not d:
                break
            spare -= len(d)
            kept.append((s, d))
        if not kept or len(kept) < self.cfg.spec_min_fraction * len(batch.decodes):
            for s, _ in cand:             # too few drafts to pay for a verify step
                s.spec_wait = 3           # (and look again in a few steps, not every step)
            return False
        drafted = []
        for s, d in kept:
            need = s.length + len(d) + 1
            extra = self.blocks.blocks_needed(need) - len(self.blocks.tables.get(s.seq_id, []))
            if extra > self.blocks.num_free:
                continue                      # no blocks for the draft: plain decode row
            self.blocks.ensure(s.seq_id, need)
            s.draft = d
            drafted.append(s)
        return bool(drafted)

    def _run_verify(self, batch: Batch) -> List[Sequence]:
        """One forward over [last token + draft] chunks of the drafted sequences and the other
        decode rows: the longest draft prefix the model's argmax agrees with is accepted, plus
        the model's own next token -- greedy outputs identical to one-token decoding."""
        drafted = [s for s in batch.decodes if s.draft]
        vb = Batch("verify", [(s, 1 + len(s.draft)) for s in drafted],
                   [s for s in batch.decodes if not s.draft])
        inp = self._build_input(vb)
        if self.tp > 1:
            self._broadcast(inp)
        logits = self.runner.execute(inp)
        # drafted rows are greedy (argmax); the undrafted decode rows keep their own sampling
        t, lp, _ = self._sample(inp, logits,
                                [s for s, c in vb.prefills for _ in range(c)] + vb.decodes)
        amv = t.tolist()
        lpv = lp.tolist() if lp is not None else [None] * len(amv)
        self.runner.check_collectives()
        self.stats["prefill_tokens"] += inp.num_prefill_rows
        self.stats["decode_tokens"] += len(vb.decodes)
        self.stats["spec_steps"] += 1
        r = 0
        out = []
        for s, c in vb.prefills:
            d, s.draft = s.draft, []
            acc = 0
            while acc < len(d) and amv[r + acc] == d[acc]:
                acc += 1
            self.stats["spec_proposed"] += len(d)
            self.stats["spec_accepted"] += acc
            if acc:
                s.spec_misses = 0
            else:
                s.spec_misses += 1
                s.spec_wait = min(2 ** s.spec_misses - 1, 63)
            for t, lp in zip(d[:acc] + [amv[r + acc]], lpv[r:r + acc + 1]):
                s.append(int(t), lp, self.eos_id)
                if s.finished:
                    break
            s.num_cached = s.length - 1       # K/V valid up to the last accepted input
            r += c
            out.append(s)
        for s in vb.decodes:
            s.num_cached = s.length
            s.append(int(amv[r]), lpv[r], self.eos_id)
            r += 1
            out.append(s)
        self.stats["finished"] += len(self.scheduler.finish(vb))
        self.stats["steps"] += 1
        self.step_count += 1
        return out

    def _extras(self, inp: StepInput, logits: torch.Tensor, sampled: List[Sequence]) -> list:
        """Host lists of the ``top_logprobs`` alternatives of each sampled row (None where not
        asked; from the distribution the row was sampled from: logits / temperature, raw when
        greedy), and the prompt scores of this step's prefill rows (stored on the sequences)."""
        tops: list = [None] * len(sampled)
        ks = [s.params.top_logprobs for s in sampled]
        if any(ks):
            z = logits.float()
            t = inp.temps.float()[:, None]
            z = torch.where(t > 0, z / t.clamp(min=1e-6), z)
            v, ix = torch.log_softmax(z, -1).topk(max(ks), -1)
            v, ix = v.tolist(), ix.tolist()
            # a guided row's masked tokens (logprob -inf) are no alternatives
            tops = [[(j, x) for j, x in zip(ix[i][:k], v[i][:k]) if x != float("-inf")] if k
                    else None for i, k in enumerate(ks)]
        meta = inp.prompt_meta
        if meta:
            lp = torch.log_softmax(self.runner.extra_logits.float(), -1)
            tgt = torch.tensor([t for s, j0, n, _ in meta for t in s.prompt_ids[j0:j0 + n]],
                               dtype=torch.long, device=lp.device)
            tl = lp.gather(1, tgt[:, None])[:, 0].tolist()
            kp = max(s.params.prompt_logprobs for s, *_ in meta)
            pv = pi = None
            if kp:
                pv, pi = lp.topk(kp, -1)
                pv, pi = pv.tolist(), pi.tolist()
            for s, j0, n, r0 in meta:
                if not s.prompt_scores:
                    s.prompt_scores.append(None)   # the first token has no prefix to score it
                k = s.params.prompt_logprobs
                for q in range(n):
                    if j0 + q != len(s.prompt_scores):
                        continue                   # scored before (recompute after preemption)
                    alts = list(zip(pi[r0 + q][:k], pv[r0 + q][:k])) if k else []
                    s.prompt_scores.append((tl[r0 + q], alts))
        return tops

    def generate(self, prompts: Iterable[Union[str, List[int]]],
                 params: Optional[SamplingParams] = None) -> List[Sequence]:
        seqs = [self.add_request(p, SamplingParams(**vars(params)) if params else None)
                for p in prompts]
        while any(not s.finished for s in seqs):
            self.step()
        return seqs

    def shutdown(self):
        if self.tp > 1:
            self._broadcast(None)


class AsyncEngine:
    """Background-thread engine loop + asyncio streaming (OpenAI server backend)."""

    def __init__(self, engine: LLMEngine):
        self.engine = engine
        self._inbox: "queue.Queue" = queue.Queue()
        self._streams: Dict[str, tuple] = {}
        self._stop = threading.Event()
        self._thread = threading.Thread(target=self._loop, name="lumen-engine", daemon=True)
        self._thread.start()

    def _loop(self):
        eng = self.engine
        while not self._stop.is_set():
            try:
                while True:
                    op = self._inbox.get_nowait()
                    if op[0] == "add":
                        _, prompt, params, rid, lora = op
                        try:
                            seq = eng.add_request(prompt, params, rid, lora)
                            self._push(rid, ("start", seq))
                        except Exception as e:  # bad request -> report to its stream
                            self._push(rid, ("error", str(e)))
                    elif op[0] == "abort":
                        eng.abort(op[1])
            except queue.Empty:
                pass
            if not eng.has_work:
                time.sleep(0.0005)
                continue
            try:
                seqs = eng.step()
            except Exception as e:  # surface engine failures to every open stream
                for rid in list(self._streams):
                    self._push(rid, ("error", repr(e)))
                raise
            for s in seqs:
                self._push(s.request_id, ("token", s))

    # -- interface shared with frontend.EngineCoreClient (what the API server reads) ---------
    @property
    def tokenizer(self):
        return self.engine.tokenizer

    @property
    def model_name(self) -> str:
        return self.engine.cfg.model

    @property
    def max_model_len(self) -> int:
        return self.engine.cfg.max_model_len

    @property
    def eos_id(self):
        return self.engine.eos_id

    def live_stats(self) -> dict:
        sch = self.engine.scheduler
        return {"kv_usage": self.engine.blocks.usage(), "running": len(sch.running),
                "waiting": len(sch.waiting), "preemptions": sch.num_preemptions,
                "prefix_hit_rate": self.engine.blocks.hit_rate, **self.engine.guided_stats()}

    @property
    def guided_max_states(self) -> int:
        return self.engine.cfg.guided_max_states

    def _push(self, rid, item):
        st = self._streams.get(rid)
        if st is None:
            return
        loop, q = st
        loop.call_soon_threadsafe(q.put_nowait, item)

    @property
    def lora_names(self) -> List[str]:
        return list(self.engine.lora_names)

    async def stream(self, prompt, params: SamplingParams, request_id: Optional[str] = None,
                     lora: Optional[str] = None):
        """Async generator of (sequence, new_token_count) updates until finished."""
        rid = request_id or uuid.uuid4().hex
        q: asyncio.Queue = asyncio.Queue()
        self._streams[rid] = (asyncio.get_running_loop(), q)
        self._inbox.put(("add", prompt, params, rid, lora))
        kind, payload = "start", None
        try:
            while True:
                kind, payload = await q.get()
                if kind == "error":
                    raise ValueError(payload)
                if kind == "start":
                    continue
                yield payload
                if payload.finished:
                    break
        finally:
            self._streams.pop(rid, None)
            if not (kind == "token" and payload is not None and payload.finished):
                self._inbox.put(("abort", rid))  # client went away: free its KV blocks

    def shutdown(self):
        self._stop.set()
        self._thread.join(timeout=5)
