"""The two kernels of the text cache (csrc/clip_text.hip): mesm_text_cache_store copies the tower's rows into slots, bit
for bit and nowhere else; mesm_text_pool_slots is mesm_text_pool reading pair n from slot slots[n] -- the same kernel body,
so words and sentence must carry the bits of mesm_text_pool on the gathered dense tensor, NaN of an all-pad row included."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (Lx, Lw, D): the released size; a small one; D no multiple of 8 halfs (the scalar path), one cached row per query
SHAPES = [(77, 32, 512), (8, 8, 64), (5, 1, 48)]
CAPACITY = 9


def _bits16(t):
    return t.contiguous().view(torch.int16)


def _bits32(t):
    return t.contiguous().view(torch.int32)


def _hid(n, Lx, D, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, Lx, D, generator=g) * 3.0).half().to(DEV)


@pytest.mark.parametrize("Lx,Lw,D", SHAPES)
@pytest.mark.parametrize("M", [1, 5])
def test_store_writes_the_named_slots_and_nothing_else(Lx, Lw, D, M):
    from mesm_amd import kernels as kn
    n = 11
    hid = _hid(n, Lx, D, 1)
    cache = _hid(CAPACITY, Lw, D, 2)  # previous contents: any bits
    before = cache.clone()
    # source rows: a permutation with gaps; slots unordered, the last and the first among them
    rows = [7, 0, 10, 3, 5][:M] if M > 1 else [10]
    slots = [CAPACITY - 1, 4, 0, 6, 2][:M] if M > 1 else [CAPACITY - 1]
    r = torch.tensor(rows, dtype=torch.int32, device=DEV)
    s = torch.tensor(slots, dtype=torch.int32, device=DEV)
    kn.text_cache_store(hid, r, s, cache, Lw)
    torch.cuda.synchronize()
    for m in range(M):
        assert torch.equal(_bits16(cache[slots[m]]), _bits16(hid[rows[m], :Lw])), (m, rows[m], slots[m])
    for k in range(CAPACITY):
        if k not in slots:
            assert torch.equal(_bits16(cache[k]), _bits16(before[k])), k
    if M == 5:
        # slot 0 and the last slot through a second call, the other way round
        kn.text_cache_store(hid, torch.tensor([1, 2], dtype=torch.int32, device=DEV),
                            torch.tensor([0, CAPACITY - 1], dtype=torch.int32, device=DEV), cache, Lw)
        assert torch.equal(_bits16(cache[0]), _bits16(hid[1, :Lw]))
        assert torch.equal(_bits16(cache[CAPACITY - 1]), _bits16(hid[2, :Lw]))
        assert torch.equal(_bits16(cache[4]), _bits16(hid[0, :Lw]))


def _masks(N, Lm, Lw):
    """a full row, a one-word row, an all-pad row, then rows of growing length"""
    m = torch.zeros(N, Lm, dtype=torch.bool)
    for i in range(N):
        k = [Lw, 1, 0][i] if i < 3 else 1 + (i * 5) % Lw
        m[i, :k] = True
    return m.to(DEV)


@pytest.mark.parametrize("Lx,Lw,D", SHAPES)
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("N", [1, 7])
def test_pool_over_slots_has_the_bits_of_pool_over_the_gathered_rows(Lx, Lw, D, normalize, N):
    from mesm_amd import kernels as kn
    cache = _hid(CAPACITY, Lw, D, 3)
    # unordered, the last and the first slot, one slot for two pairs
    slots = [CAPACITY - 1, 0, 4, 4, 2, 7, 0][:N] if N > 1 else [CAPACITY - 1]
    sl = torch.tensor(slots, dtype=torch.int32, device=DEV)
    Lm = Lx  # the batch's mask keeps the collate's extent
    mask = _masks(N, Lm, Lw)
    if N == 1:
        mask[0, Lw // 2 + 1:] = False
    words, sent = kn.text_pool_slots(cache, sl, mask, normalize)
    dense = cache[sl.long()].contiguous()
    words_d, sent_d = kn.text_pool(dense, mask, Lw, normalize)
    torch.cuda.synchronize()
    assert words.shape == (N, Lw, D) and sent.shape == (N, D) and words.dtype == sent.dtype == torch.float32
    assert torch.equal(_bits32(words), _bits32(words_d))
    assert torch.equal(_bits32(sent), _bits32(sent_d))
    if N > 1:
        # the all-pad row divides by a zero count: its sentence is NaN in both, its words zero
        assert bool(torch.isnan(sent[2]).all()) and float(words[2].abs().max()) == 0.0
        # two pairs on one slot under different masks are their own results
        assert not torch.equal(sent[2], sent[3])


def test_store_then_pool_is_the_uncached_text_stage():
    """the two kernels in the order the model uses them, at the released size: tower rows -> slots -> pooled"""
    from mesm_amd import kernels as kn
    Lx, Lw, D, N = 77, 32, 512, 6
    hid = _hid(N, Lx, D, 5)
    cache = torch.zeros(CAPACITY, Lw, D, dtype=torch.float16, device=DEV)
    slots = [3, 8, 0, 5, 1, 6]
    sl = torch.tensor(slots, dtype=torch.int32, device=DEV)
    kn.text_cache_store(hid, torch.arange(N, dtype=torch.int32, device=DEV), sl, cache, Lw)
    mask = _masks(N, Lx, Lw)
    words, sent = kn.text_pool_slots(cache, sl, mask, True)
    words_d, sent_d = kn.text_pool(hid, mask, Lw, True)
    assert torch.equal(_bits32(words), _bits32(words_d)) and torch.equal(_bits32(sent), _bits32(sent_d))


def test_out_of_range_indices_are_clamped_to_the_buffers():
    """whatever the index arrays hold, the kernels stay inside the two buffers (the rule of optim.hip's tables)"""
    from mesm_amd import kernels as kn
    Lx, Lw, D = 8, 8, 64
    hid = _hid(3, Lx, D, 6)
    cache = torch.zeros(4, Lw, D, dtype=torch.float16, device=DEV)
    kn.text_cache_store(hid, torch.tensor([99, -5], dtype=torch.int32, device=DEV),
                        torch.tensor([77, -1], dtype=torch.int32, device=DEV), cache, Lw)
    torch.cuda.synchronize()
    assert torch.equal(_bits16(cache[3]), _bits16(hid[2])) and torch.equal(_bits16(cache[0]), _bits16(hid[0]))
    assert float(cache[1:3].abs().max()) == 0.0
    mask = torch.ones(2, Lw, dtype=torch.bool, device=DEV)
    words, _ = kn.text_pool_slots(cache, torch.tensor([1000, -7], dtype=torch.int32, device=DEV), mask, False)
    assert torch.equal(words[0], cache[3].float()) and torch.equal(words[1], cache[0].float())
