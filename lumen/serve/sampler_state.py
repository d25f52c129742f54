"""Per-sequence sampling state on the device (kernels/sampling_rows.hip).

``SamplerState`` is the count table behind the penalties: one int32 row of V entries per
running sequence that has a penalty (bit 31 = "in the prompt", bits 0..30 = times generated).
The sampling kernel reads the row while it processes the logits and bumps the sampled token's
entry itself, so a penalised request needs no token values on the host and keeps async
scheduling.  The table is allocated at the first request with a penalty
(``max_num_seqs * V * 4`` bytes: 32.8 MB at 256 x 32000); an engine that never sees one
allocates nothing.  Owned by the engine on rank 0 -- TP workers never sample.

``RowParams`` carries the per-row arguments of a step that uses the per-row sampler entry: on
the device (slices of the engine's packed step copy) when the native extension samples, as
host arrays for the torch reference.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch


@dataclass
class RowParams:
    seed: object                 # [R] int64
    offset: object               # [R] int64
    rngrow: object               # [R] int64
    min_p: object                # [R] f32
    slot: object                 # [R] int32, -1 = no state
    rp: object                   # [R] f32 repetition / frequency / presence penalties
    fp: object
    pp: object
    bias_ptr: Optional[object] = None   # CSR over the rows, int32 [R + 1] (None: no entries)
    bias_idx: Optional[object] = None   # int32
    bias_val: Optional[object] = None   # f32 (-inf: banned)
    g_table: Optional[object] = None    # [R] int64 address of the row's token table, 0 = unguided
    g_slot: Optional[object] = None     # [R] int32 row of GuidedState.state
    host: dict = field(default_factory=dict)   # the same arrays as numpy (CPU reference path)


class SamplerState:
    def __init__(self, num_slots: int, vocab: int, device: torch.device):
        self.num_slots, self.vocab, self.device = num_slots, vocab, device
        self.counts: Optional[torch.Tensor] = None
        self.free: List[int] = list(range(num_slots - 1, -1, -1))

    @property
    def allocated(self) -> bool:
        return self.counts is not None

    @property
    def num_free(self) -> int:
        return len(self.free)

    def acquire(self) -> int:
        if self.counts is None:
            self.counts = torch.zeros(self.num_slots, self.vocab, dtype=torch.int32,
                                      device=self.device)
        return self.free.pop()

    def release(self, seq) -> None:
        """Called wherever the scheduler releases a sequence (finish, abort, preemption).
        Nothing is cleared here, and the slot may be handed out again at once: stream order
        makes the reuse safe.  The next owner's init launch zeroes the row, and it is enqueued
        after every sampler launch that could still write the old owner's row -- including the
        row a step already in flight samples for a sequence whose EOS is seen one step late."""
        if seq.state_slot >= 0:
            self.free.append(seq.state_slot)
            seq.state_slot = -1

    def init_slots(self, slots, ptr, n_prompt, ids) -> None:
        """Device int32 tensors: new slots [n], CSR ptr [n + 1], prompt lengths [n], ids."""
        from ..ops._native import native

        native().sampler_state_init(self.counts, slots, ptr, n_prompt, ids, slots.numel())


class GuidedState:
    """The automaton state of every running guided sequence: one int32 per slot, on the engine's
    device (a CPU tensor for the CPU engine).  The sampling launch reads a row's state to mask
    the logits and stores the successor after the draw, so guided requests keep async
    scheduling.  Allocated at the first guided request; slots are handed out and returned like
    ``SamplerState``'s (stream order makes the reuse safe: the next owner's state is written by
    a copy enqueued after every launch that could still advance the old owner's)."""

    def __init__(self, num_slots: int, device: torch.device):
        self.num_slots, self.device = num_slots, device
        self.state: Optional[torch.Tensor] = None
        self.free: List[int] = list(range(num_slots - 1, -1, -1))

    @property
    def num_free(self) -> int:
        return len(self.free)

    def acquire(self) -> int:
        if self.state is None:
            self.state = torch.zeros(self.num_slots, dtype=torch.int32, device=self.device)
        return self.free.pop()

    def release(self, seq) -> None:
        if seq.guided_slot >= 0:
            self.free.append(seq.guided_slot)
            seq.guided_slot = -1
        if seq.guided_table is not None and seq.finished:
            seq.guided_table.refs -= 1
            seq.guided_table = None

    def write(self, slots: torch.Tensor, states: torch.Tensor) -> None:
        """int64 slots [n] and int32 states [n] on the device: the newly admitted sequences."""
        self.state.index_copy_(0, slots, states)


def advance_guided_ref(state: torch.Tensor, tables, slots, tokens) -> None:
    """Torch reference of the kernel's state update: state[slot] = next[state][token] when that
    is >= 0.  ``tables``: the row's token table tensor or None."""
    for i, nx in enumerate(tables):
        if nx is None:
            continue
        n = int(nx[int(state[slots[i]]), int(tokens[i])])
        if n >= 0:
            state[slots[i]] = n


def counts_from_ids(prompt_ids, output_ids, vocab: int) -> torch.Tensor:
    """The count row of a sequence from its host ids (torch reference of the init kernel)."""
    c = torch.zeros(vocab, dtype=torch.int64)
    p = torch.as_tensor(list(prompt_ids), dtype=torch.long)
    p = p[(p >= 0) & (p < vocab)]
    c[p] = 1 << 31
    o = torch.as_tensor(list(output_ids), dtype=torch.long)
    o = o[(o >= 0) & (o < vocab)]
    c += torch.bincount(o, minlength=vocab)
    return c


def bias_csr(entries: List[Optional[tuple]]):
    """[(idx int64 array, val float64 array) or None per row] -> (ptr, idx, val) numpy."""
    n = np.fromiter((0 if e is None else len(e[0]) for e in entries), np.int64, len(entries))
    ptr = np.zeros(len(entries) + 1, dtype=np.int64)
    np.cumsum(n, out=ptr[1:])
    live = [e for e in entries if e is not None and len(e[0])]
    if not live:
        return ptr, np.zeros(0, np.int64), np.zeros(0, np.float64)
    return (ptr, np.concatenate([e[0] for e in live]), np.concatenate([e[1] for e in live]))
