"""The host table of the text cache (mesm_amd/textcache.py) alone, no device: slots for hits, misses and duplicates, LRU
order, the never-evict-the-current-batch rule, the refusal of a batch with more distinct queries than slots, invalidation
and the counters.  The slot tensor is taken as given (its contents belong to tests/test_text_cache_kernels_gpu.py)."""
import numpy as np
import pytest
import torch

from mesm_amd.textcache import TextCache

CTX = 7


def q(*names):
    """token-id rows (len(names), CTX) int64: one distinct row per name"""
    return np.stack([np.full(CTX, n, dtype=np.int64) for n in names])


def make(capacity):
    return TextCache(capacity, 4, 8, "cpu")


def test_state_is_one_preallocated_half_tensor():
    tc = make(5)
    assert tc.data.shape == (5, 4, 8) and tc.data.dtype == torch.float16
    addr = tc.data.data_ptr()
    tc.lookup(q(1, 2, 3))
    tc.clear()
    tc.lookup(q(4))
    assert tc.data.data_ptr() == addr
    with pytest.raises(ValueError):
        make(0)


def test_hits_misses_and_duplicates_in_one_batch():
    tc = make(8)
    slots, rows, dst = tc.lookup(q(1, 2, 1, 3, 2, 1))
    assert slots.dtype == np.int32 and slots.shape == (6,)
    assert slots[0] == slots[2] == slots[5] and slots[1] == slots[4]
    assert len({int(slots[0]), int(slots[1]), int(slots[3])}) == 3
    # every missed key once: its first row, its slot
    assert rows == [0, 1, 3] and dst == [int(slots[0]), int(slots[1]), int(slots[3])]
    assert tc.stats() == {"hits": 0, "misses": 6, "encoded_rows": 3, "evictions": 0, "entries": 3, "capacity": 8,
                          "generation": 0}
    slots2, rows2, dst2 = tc.lookup(q(3, 1, 4, 4))
    assert slots2[0] == slots[3] and slots2[1] == slots[0] and slots2[2] == slots2[3]
    assert rows2 == [2] and dst2 == [int(slots2[2])] and int(slots2[2]) not in set(slots.tolist())
    s = tc.stats()
    assert (s["hits"], s["misses"], s["encoded_rows"], s["entries"], s["evictions"]) == (2, 8, 4, 4, 0)
    # the key is the whole row: a row that differs in its last id is another query
    other = q(1)
    other[0, -1] = 99
    _, rows3, _ = tc.lookup(other)
    assert rows3 == [0]
    # tensors are taken like arrays
    slots4, rows4, _ = tc.lookup(torch.from_numpy(q(1, 3)))
    assert rows4 == [] and slots4.tolist() == [int(slots[0]), int(slots[3])]


def test_least_recently_used_goes_first_over_several_batches():
    tc = make(3)
    s1, _, _ = tc.lookup(q(1, 2, 3))
    slot = dict(zip((1, 2, 3), s1.tolist()))
    tc.lookup(q(1))           # order of use now 2, 3, 1
    s4, rows, dst = tc.lookup(q(4))
    assert rows == [0] and dst == [slot[2]] and s4.tolist() == [slot[2]]  # 2 was the oldest
    tc.lookup(q(3))           # order 1, 4, 3
    s5, _, dst = tc.lookup(q(5))
    assert dst == [slot[1]]
    _, rows, _ = tc.lookup(q(4, 3, 5))
    assert rows == []         # all three still there
    _, rows, _ = tc.lookup(q(2))
    assert rows == [0]        # 2 was evicted and comes back as a miss
    s = tc.stats()
    assert s["evictions"] == 3 and s["entries"] == 3


def test_a_key_of_the_current_batch_is_never_evicted():
    tc = make(3)
    s0, _, _ = tc.lookup(q(1, 2, 3))
    slot = dict(zip((1, 2, 3), s0.tolist()))
    # 1 is the least recently used entry, but the batch uses it: the two new keys must take the slots of 2 and 3
    s, rows, dst = tc.lookup(q(4, 1, 5))
    assert s[1] == slot[1] and sorted(dst) == sorted([slot[2], slot[3]]) and rows == [0, 2]
    assert len(set(s.tolist())) == 3
    # a full-capacity batch of new keys replaces everything, each slot once
    s, rows, dst = tc.lookup(q(7, 8, 9))
    assert sorted(s.tolist()) == [0, 1, 2] and rows == [0, 1, 2]


def test_more_distinct_keys_than_slots_raises_before_any_change():
    tc = make(2)
    tc.lookup(q(1, 2))
    before = (tc.stats(), list(tc.table.items()), list(tc.free), tc.version)
    with pytest.raises(ValueError, match="3 distinct.*capacity 2"):
        tc.lookup(q(1, 3, 4))
    assert (tc.stats(), list(tc.table.items()), list(tc.free), tc.version) == before
    # duplicates do not count: two distinct keys in four rows fit
    s, _, _ = tc.lookup(q(5, 6, 5, 6))
    assert s[0] == s[2] and s[1] == s[3] and s[0] != s[1]


def test_invalidation_empties_the_table_and_bumps_the_generation():
    tc = make(4)
    tc.lookup(q(1, 2), source_generation=10)
    _, rows, _ = tc.lookup(q(1, 2), source_generation=10)
    assert rows == [] and tc.stats()["generation"] == 0
    # the text encoder's generation moved: the next lookup starts from an empty table
    _, rows, _ = tc.lookup(q(1, 2), source_generation=11)
    assert rows == [0, 1]
    s = tc.stats()
    assert s["generation"] == 1 and s["entries"] == 2 and s["evictions"] == 0
    tc.clear()
    s = tc.stats()
    assert s["generation"] == 2 and s["entries"] == 0 and s["evictions"] == 0
    slots, rows, _ = tc.lookup(q(3, 1), source_generation=11)
    assert rows == [0, 1] and sorted(slots.tolist()) == [0, 1]
    assert tc.stats()["encoded_rows"] == 6 and tc.stats()["hits"] == 2 and tc.stats()["misses"] == 6


def test_the_model_switch_refuses_models_without_a_clip_tower_and_keeps_the_cache_out_of_the_state_dict():
    from mesm_amd import build_model, synthetic
    args = synthetic.make_args("C3b", device="cpu")
    model = build_model(args)  # pre-extracted word features: no text encoder
    with pytest.raises(ValueError, match="no text encoder"):
        model.text_cache(16)
    assert model.text_cache(None) is None and model.text_cache_stats() is None
