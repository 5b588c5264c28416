"""The frozen CLIP text tower's outputs, cached on the device per query.

The tower (text_encoder.CLIPTextEncoder) is frozen, fp16, without dropout: the first `Lw` rows of a query's
`last_hidden_state` are a function of its token ids alone, and a training run meets the same few thousand queries for
hundreds of epochs.  A `TextCache` keeps those rows, as the tower wrote them, in ONE preallocated fp16 tensor
(capacity, Lw, width) whose address never moves -- a captured graph reads it through a static int32 slot array
(`mesm_text_pool_slots`) -- and a host table from a query's key to its slot:

    key        the bytes of the query's full int64 token-id row (all context_length ids)
    eviction   least recently used first; a key of the batch being looked up is never evicted
    invalid    whenever the tower's weights may have changed (`lookup(..., source_generation=...)` with another number
               than the last one, or `clear()`): the table starts empty, nothing counts as an eviction

Pooling and normalisation are not cached: they depend on the batch's mask and on `normalize_txt`, cost one launch, and
re-evaluated from the cached rows they are the arithmetic of the uncached path, bit for bit.  The table is host state of
the training process; the cache is derived data and belongs to no state_dict.
"""
from collections import OrderedDict

import numpy as np
import torch


class TextCache:
    def __init__(self, capacity, Lw, width, device):
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("TextCache: capacity must be at least 1, got %d" % capacity)
        self.capacity, self.Lw, self.width = capacity, int(Lw), int(width)
        self.device = torch.device(device)
        # (zeros, not empty: a slot that was never stored holds finite values whatever reads it)
        self.data = torch.zeros(capacity, self.Lw, self.width, dtype=torch.float16, device=self.device)
        self.table = OrderedDict()  # key -> slot, least recently used first
        self.free = list(range(capacity - 1, -1, -1))  # (pop() hands out slot 0 first)
        self.generation = 0
        self.version = 0  # grows whenever a key may have moved to another slot (a miss placed, the table emptied)
        self._source_gen = None
        self.hits = self.misses = self.encoded_rows = self.evictions = 0

    # ------------------------------------------------------------------ invalidation
    def clear(self):
        """forget every entry (the tower's weights changed): an empty table, the next generation, no evictions counted"""
        self.table.clear()
        self.free = list(range(self.capacity - 1, -1, -1))
        self.generation += 1
        self.version += 1

    def sync(self, source_generation):
        """clear() when the text encoder's generation is not the one the entries were made under"""
        if source_generation != self._source_gen:
            if self._source_gen is not None or self.table:
                self.clear()
            self._source_gen = source_generation

    # ------------------------------------------------------------------ the host table
    @staticmethod
    def keys_of(ids_host):
        a = ids_host.detach().cpu().numpy() if torch.is_tensor(ids_host) else np.asarray(ids_host)
        if a.ndim != 2:
            raise ValueError("TextCache.lookup: token ids (N, context_length), got shape %s" % (tuple(a.shape),))
        a = np.ascontiguousarray(a, dtype=np.int64)
        return [a[i].tobytes() for i in range(a.shape[0])]

    def lookup(self, ids_host, source_generation=None):
        """ids_host (N, context_length) int64 on the host -> (slots int32[N], miss_rows, miss_slots): the slot of every
        row, and for every key that was not in the table the first row that carries it and the slot it was given -- the
        caller encodes exactly these rows and stores them before anything reads `slots`.  Duplicate keys share a slot.
        hits / misses count rows (a key's repeats inside the batch count like its first row), encoded_rows the keys
        handed out as misses.  ValueError, before anything changes, when the batch has more distinct keys than slots."""
        keys = self.keys_of(ids_host)
        distinct = list(OrderedDict.fromkeys(keys))
        if len(distinct) > self.capacity:
            raise ValueError("TextCache: %d distinct queries in one batch, capacity %d" % (len(distinct), self.capacity))
        if source_generation is not None:
            self.sync(source_generation)
        table = self.table
        known = {k for k in distinct if k in table}
        for k in distinct:  # the batch's own keys first: they end up behind everything an eviction may take
            if k in known:
                table.move_to_end(k)
        first = {}
        for i, k in enumerate(keys):
            first.setdefault(k, i)
        miss_rows, miss_slots = [], []
        for k in distinct:
            if k in known:
                continue
            if self.free:
                s = self.free.pop()
            else:
                # the front of the table is no key of this batch: those were moved (hits) or appended (misses) behind
                # it, and there are fewer of them than slots
                _, s = table.popitem(last=False)
                self.evictions += 1
            table[k] = s
            miss_rows.append(first[k])
            miss_slots.append(s)
        slots = np.fromiter((table[k] for k in keys), dtype=np.int32, count=len(keys))
        n_hit = sum(1 for k in keys if k in known)
        self.hits += n_hit
        self.misses += len(keys) - n_hit
        self.encoded_rows += len(miss_rows)
        if miss_rows:
            self.version += 1
        return slots, miss_rows, miss_slots

    def stats(self):
        return {"hits": self.hits, "misses": self.misses, "encoded_rows": self.encoded_rows, "evictions": self.evictions,
                "entries": len(self.table), "capacity": self.capacity, "generation": self.generation}

    # ------------------------------------------------------------------ the device side
    def store(self, hid, miss_slots):
        """hid (M, Lx, width) fp16, the tower's output for the missing rows: hid[m, :Lw] -> slot miss_slots[m], on the
        current stream"""
        from . import kernels as kn
        M = len(miss_slots)
        if M == 0:
            return
        idx = np.empty((2, M), dtype=np.int32)
        idx[0] = np.arange(M)
        idx[1] = miss_slots
        dev = torch.from_numpy(idx).to(self.device, non_blocking=False)
        kn.text_cache_store(hid, dev[0], dev[1], self.data, self.Lw)
