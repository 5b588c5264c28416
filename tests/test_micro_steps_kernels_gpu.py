"""The device side of micro-batched graph replays (include/mesm_gfx950.h: mesm_micro_begin, mesm_fill_ranges_gated,
mesm_grad_sumsq_gated, mesm_adamw_step_gated, mesm_adamw_step_groups_gated) on buffers of a few thousand floats: the cycle
words follow the host formula, the gated fill and the gated optimizer launches write nothing when their gate is closed and
give the ungated entries' bits when it is open."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

N = 4 * 1237  # 1237 groups of 4: more than one workgroup of 256 threads (five), the last one partly filled
SEGMENTS = (1, 1, 2, 16, 75, 37)  # run lengths in groups of 4 (132 in all): boundaries fall inside a wave
GROUPS = ((1e-3, (0.9, 0.999), 1e-8, 1e-2, 0),
          (1e-4, (0.8, 0.99), 1e-6, 0.0, 2),
          (0.0, (0.9, 0.999), 1e-8, 0.1, 0))


def dev():
    return torch.device("cuda:0")


def _words(count=0, k=1, phase=0, due=0):
    return torch.tensor([count, k, phase, due], dtype=torch.int32, device=dev())


def _tags(values):
    n4 = N // 4
    lens = torch.tensor(SEGMENTS * (n4 // sum(SEGMENTS) + 1))
    vals = torch.tensor([values[j % len(values)] for j in range(len(lens))], dtype=torch.uint8)
    return torch.repeat_interleave(vals, lens)[:n4].contiguous().to(dev())


def _table(rows):
    from mesm_amd import _lib
    arr = (_lib.AdamGroup * len(rows))()
    for r, (lr, (b1, b2), eps, wd, step0) in zip(arr, rows):
        r.lr, r.beta1, r.beta2, r.eps, r.weight_decay, r.step0 = lr, b1, b2, eps, wd, step0
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev())


@functools.lru_cache(maxsize=None)
def _inputs():
    """(p, g, m, v), gradient magnitudes log-uniform in 1e-4..1; never modified (the tests work on clones)"""
    gen = torch.Generator(device=dev()).manual_seed(5)
    rnd = lambda f: f(N, device=dev(), generator=gen, dtype=torch.float32)
    p, m, v = rnd(torch.randn), 0.1 * rnd(torch.randn), 0.01 * rnd(torch.rand)
    mag = torch.pow(10.0, -4.0 * rnd(torch.rand))
    g = torch.where(rnd(torch.rand) < 0.5, -mag, mag)
    return p, g, m, v


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_tag_boundaries_fall_inside_a_wave_and_sizes_are_off_the_grid_stride():
    tags = _tags((1, 2, 3, 0)).long()
    starts = torch.nonzero(tags[1:] != tags[:-1]).flatten() + 1
    assert bool((starts % 64 != 0).any()) and (N // 4) % 256 != 0 and N // 4 > 256
    assert set(tags.tolist()) == {0, 1, 2, 3}


def test_gated_fill_clears_on_phase_zero_only():
    from mesm_amd._lib import check, lib, ptr, stream_ptr
    gen = torch.Generator(device=dev()).manual_seed(1)
    buf = torch.randn(6000, device=dev(), generator=gen) + 3.0  # (no zero in it)
    before = buf.clone()
    # two ranges, 16-byte aligned, of 1237 and 300 vectors of 16 bytes, with untouched floats on every side of them
    ranges = ((8, 4 * 1237), (5200, 4 * 75))
    ptrs = (ctypes.c_void_p * 2)(*[buf.data_ptr() + 4 * o for o, _ in ranges])
    nb = (ctypes.c_int64 * 2)(*[4 * n for _, n in ranges])
    for phase in (1, 2, -1):
        w = _words(phase=phase)
        check(lib().mesm_fill_ranges_gated(ptrs, nb, 2, ptr(w[2:3]), stream_ptr()), "gated fill")
        torch.cuda.synchronize()
        assert torch.equal(_bits(buf), _bits(before)), phase
    w = _words(count=1, k=3, phase=0, due=1)  # only the phase word counts
    check(lib().mesm_fill_ranges_gated(ptrs, nb, 2, ptr(w[2:3]), stream_ptr()), "gated fill")
    torch.cuda.synchronize()
    inside = torch.zeros(6000, dtype=torch.bool, device=dev())
    for o, n in ranges:
        inside[o:o + n] = True
    assert int(buf[inside].abs().sum()) == 0 and int((buf[inside].view(torch.int32) != 0).sum()) == 0
    assert torch.equal(_bits(buf[~inside]), _bits(before[~inside]))
    assert w.tolist() == [1, 3, 0, 1]  # the fill reads the state, it never writes it
    assert lib().mesm_fill_ranges_gated(ptrs, nb, 2, None, None) == -1


def test_micro_begin_follows_the_host_formula():
    from mesm_amd import kernels as kn
    k = 3
    w = _words(k=k)
    seed = torch.tensor([41], dtype=torch.int32, device=dev())
    n = 0
    for _ in range(2 * k + 1):
        kn.micro_begin(w, seed)
        phase = n % k
        n += 1
        assert w.tolist() == [n % k, k, phase, int(phase == k - 1)], n
        assert int(seed) == 41 + n
    # the cycle that is under way ends, then k is rewritten at the boundary
    while n % k:
        kn.micro_begin(w, seed)
        n += 1
    assert w.tolist()[0] == 0 and w.tolist()[3] == 1
    k2, base = 2, n
    w[1:2].fill_(k2)
    for _ in range(2 * k2 + 1):
        kn.micro_begin(w, seed)
        phase = (n - base) % k2
        n += 1
        assert w.tolist() == [(n - base) % k2, k2, phase, int(phase == k2 - 1)], n
        assert int(seed) == 41 + n
    # k = 1: every replay is first and last; no seed counter given: only the words move
    w = _words(k=1)
    for _ in range(3):
        kn.micro_begin(w)
        assert w.tolist() == [0, 1, 0, 1]


def _sumsq(g, step_t, due=None):
    from mesm_amd._lib import check, lib, ptr, stream_ptr
    partials = torch.full((1024,), -7.0, device=dev(), dtype=torch.float32)
    n_p = ctypes.c_int32(0)
    if due is None:
        check(lib().mesm_grad_sumsq(ptr(g), g.numel(), ptr(partials), ctypes.byref(n_p), ptr(step_t), stream_ptr()), "sumsq")
    else:
        check(lib().mesm_grad_sumsq_gated(ptr(g), g.numel(), ptr(partials), ctypes.byref(n_p), ptr(step_t), ptr(due),
                                          stream_ptr()), "sumsq gated")
    return partials, n_p.value


def _update(form, due, max_norm=0.1):
    """one clip + update on fresh copies of the shared inputs through the ungated (due None) or the gated entries ->
    every buffer the launches may write, and the inputs"""
    from mesm_amd._lib import check, lib, ptr, stream_ptr
    p, g, m, v = (t.clone() for t in _inputs())
    step_t = torch.tensor([3], dtype=torch.int32, device=dev())
    norm = torch.full((1,), -1.0, device=dev(), dtype=torch.float32)
    partials, n_p = _sumsq(g, step_t, due)
    assert n_p == 5
    if form == "groups":
        tags, table = _tags((1, 2, 3, 0)), _table(GROUPS)
        args = (ptr(p), ptr(g), ptr(m), ptr(v), ptr(tags), N, ptr(partials), n_p, max_norm, ptr(table), len(GROUPS),
                ptr(step_t), ptr(norm))
        if due is None:
            check(lib().mesm_adamw_step_groups(*args, stream_ptr()), "groups")
        else:
            check(lib().mesm_adamw_step_groups_gated(*args, ptr(due), stream_ptr()), "groups gated")
    else:
        active = (_tags((1, 2, 3, 0)) != 0).to(torch.uint8)  # the gap of tag 0 is a tensor without a gradient
        lr_t = torch.full((1,), 1e-3, device=dev())
        args = (ptr(p), ptr(g), ptr(m), ptr(v), ptr(active), N, ptr(partials), n_p, max_norm, ptr(lr_t), 0.9, 0.999, 1e-8,
                1e-2, ptr(step_t), ptr(norm))
        if due is None:
            check(lib().mesm_adamw_step(*args, stream_ptr()), "default")
        else:
            check(lib().mesm_adamw_step_gated(*args, ptr(due), stream_ptr()), "default gated")
    torch.cuda.synchronize()
    return dict(p=p, m=m, v=v, step=step_t, norm=norm, partials=partials[:n_p].clone())


@pytest.mark.parametrize("form", ["default", "groups"])
def test_gated_update_on_a_due_replay_gives_the_ungated_bits(form):
    ref = _update(form, None)
    got = _update(form, _words(count=0, k=3, phase=2, due=1)[3:4])
    for name in ref:
        assert torch.equal(_bits(got[name]), _bits(ref[name])), name
    assert int(ref["step"]) == 4 and float(ref["norm"]) > 0.1  # (the clip acts)
    p0 = _inputs()[0]
    assert not torch.equal(got["p"], p0)
    gap = torch.repeat_interleave(_tags((1, 2, 3, 0)) == 0, 4)
    assert torch.equal(_bits(got["p"][gap]), _bits(p0[gap]))  # tag 0 stays as it is


@pytest.mark.parametrize("form", ["default", "groups"])
def test_gated_update_on_a_replay_that_is_not_due_touches_nothing(form):
    got = _update(form, _words(count=2, k=3, phase=1, due=0)[3:4])
    p, g, m, v = _inputs()
    for name, t in (("p", p), ("m", m), ("v", v)):
        assert torch.equal(_bits(got[name]), _bits(t)), name
    assert int(got["step"]) == 3
    assert float(got["norm"]) == -1.0
    assert bool((got["partials"] == -7.0).all())


def test_gated_entries_refuse_a_missing_gate():
    from mesm_amd._lib import lib, ptr
    p, g, m, v = _inputs()
    step_t = torch.zeros(1, dtype=torch.int32, device=dev())
    n_p = ctypes.c_int32(0)
    partials = torch.zeros(1024, device=dev())
    assert lib().mesm_grad_sumsq_gated(ptr(g), N, ptr(partials), ctypes.byref(n_p), ptr(step_t), None, None) == -1
    assert lib().mesm_micro_begin(None, None, None) == -1
