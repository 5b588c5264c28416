"""mesm_tensor_stats (include/mesm_gfx950.h): per-segment sum of squares in fp64 and largest magnitude as bits of the flat
gradient and parameter buffers, through direct ctypes calls.  Inputs, sizes and segment tables are those of
tests/test_guard_kernels_gpu.py ("fine" at every size: 11 933 segments at the largest; "coarse" at the largest), plus two
tables for the paths of this kernel that those do not reach: "ones" (65 536 segments of one float4: every workgroup's range
meets 1024 segments, two LDS windows of 512) and "gaps" (empty segments, and elements in front of the first and behind the
last segment that no segment holds).

Bounds.  absmax is compared bit for bit with numpy's max of view(uint32) & 0x7fffffff.  The squares of floats are exact and
non-negative in fp64, so any summation order of n of them errs by at most (n - 1) * 2^-53 relative; the numpy reference
gets the same allowance: |sumsq - ref| <= n * 2^-52 * ref per segment, n the elements of the segment."""
import functools

import numpy as np
import pytest
import torch

import test_ema_kernels_gpu as K
import test_guard_kernels_gpu as G

pytestmark = pytest.mark.gpu

SIZES = K.SIZES
N_ONES = 4 * 65536
TABLES = list(G.TABLES) + [(N_ONES, "ones"), (SIZES[1], "gaps")]
LDS_SEGS = 512  # csrc/optim.hip: STATS_LDS_SEGS
EINVAL, EALIGN = -1, -2
dev = K.dev


@functools.lru_cache(maxsize=None)
def _starts(n, kind):
    if kind == "ones":
        return np.arange(n // 4 + 1, dtype=np.int64)
    if kind == "gaps":
        return np.array([5, 5, 100, 100, 100, 300, 301, 350, 400, n // 4 - 7], dtype=np.int64)
    return G._starts(n, kind)


@functools.lru_cache(maxsize=None)
def _table(n, kind):
    return torch.tensor(_starts(n, kind), dtype=torch.int32).to(dev())


def _workgroups(n):
    from mesm_amd._lib import lib
    return int(lib().mesm_tensor_stats_workgroups(n))


class Rig:
    """the state words and the two result tables of one segment table, on the device"""

    def __init__(self, n, kind, every=1, fill=None):
        self.n, self.kind = n, kind
        self.table, self.starts = _table(n, kind), _starts(n, kind)
        self.n_seg = len(self.starts) - 1
        self.wg = _workgroups(n)
        slots = 2 * (self.n_seg + self.wg)
        self.state = torch.tensor([every, 0, 0, 0], dtype=torch.int32, device=dev())
        self.sumsq = torch.zeros(slots, dtype=torch.float64, device=dev())
        self.absmax = torch.zeros(slots, dtype=torch.int32, device=dev())
        if fill is not None:  # sentinels in every word the launch may write
            self.state[1:] = fill
            self.sumsq.view(torch.int64).fill_(0x7ff8dead0000beef)
            self.absmax.fill_(fill)

    def launch(self, g, p, index, due=None):
        from mesm_amd._lib import check, lib, ptr, stream_ptr
        idx = torch.tensor([index], dtype=torch.int32, device=dev())
        check(lib().mesm_tensor_stats(ptr(g), ptr(p), self.n, ptr(self.table), self.n_seg, ptr(due), ptr(idx), ptr(self.state),
                                      ptr(self.sumsq), ptr(self.absmax), stream_ptr()), "mesm_tensor_stats")
        torch.cuda.synchronize()
        return self

    def words(self):
        return [self.state.clone(), self.sumsq.view(torch.int64).clone(), self.absmax.clone()]

    def result(self):
        from mesm_amd.optim import reduce_stat_slots
        return reduce_stat_slots(self.starts, self.n // 4, self.wg, self.sumsq.cpu().numpy(),
                                 self.absmax.cpu().numpy().view(np.uint32))


def _reference(x, starts):
    """per segment: numpy's sum of x.astype(np.float64) ** 2 and its max of view(uint32) & 0x7fffffff (add.reduceat and
    maximum.reduceat over [start, end) pairs: one call for up to 65 536 segments); an empty segment gives 0"""
    with np.errstate(invalid="ignore", over="ignore"):  # (widening a signalling NaN raises the invalid flag)
        sq = np.append(x.astype(np.float64) ** 2, 0.0)  # (one more entry: the end of the last segment is an index too)
    bits = np.append(x.view(np.uint32) & np.uint32(0x7fffffff), np.uint32(0))
    full = starts[1:] > starts[:-1]
    pairs = np.stack([4 * starts[:-1][full], 4 * starts[1:][full]], axis=1).ravel()
    s, m = np.zeros(len(starts) - 1, dtype=np.float64), np.zeros(len(starts) - 1, dtype=np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        s[full] = np.add.reduceat(sq, pairs)[::2]
    m[full] = np.maximum.reduceat(bits, pairs)[::2]
    return s, m


@functools.lru_cache(maxsize=None)
def _inputs_np(n):
    p, g = K._inputs(n)[:2]
    return g.cpu().numpy(), p.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _input_reference(n, kind):
    """the fp64 reference of the shared inputs, computed once per table; never modified"""
    g, p = _inputs_np(n)
    return _reference(g, _starts(n, kind)), _reference(p, _starts(n, kind))


def _check(result, refs, starts, what):
    sumsq, absmax = result
    n_el = 4.0 * np.diff(starts)
    for x, (ref_s, ref_m) in enumerate(refs):
        assert np.array_equal(absmax[x], ref_m), (what, "gp"[x], "absmax")
        fin = np.isfinite(ref_s)
        err = np.abs(sumsq[x][fin] - ref_s[fin])
        bound = n_el[fin] * 2.0 ** -52 * ref_s[fin]
        worst = float(np.max(err / np.maximum(bound, 1e-300))) if fin.any() else 0.0
        print("%s %s: worst error / bound %.3g over %d segments" % (what, "gp"[x], worst, int(fin.sum())))
        assert bool(np.all(err <= bound)), (what, "gp"[x], worst)
        assert np.array_equal(np.isnan(sumsq[x]), np.isnan(ref_s)), (what, "gp"[x], "NaN")
        assert np.array_equal(np.isposinf(sumsq[x]), np.isposinf(ref_s)), (what, "gp"[x], "inf")


def test_tables_are_where_the_kernel_can_go_wrong():
    assert [_workgroups(n) for n in SIZES] == [1, 1, 257] and _workgroups(N_ONES) == 64
    assert _workgroups(4 * 1024 * 1024 * 3 + 4) == 1024  # the cap
    assert _workgroups(0) == EINVAL and _workgroups(6) == EINVAL
    for n, kind in TABLES:
        s = _starts(n, kind)
        assert 0 <= s[0] and s[-1] <= n // 4 and bool(np.all(np.diff(s) >= 0))
    # one workgroup with all its segments in one window; 257 workgroups whose borders fall inside segments (1022 float4
    # each: no multiple of the tables' period of 132) and whose slots are offset by the workgroup index; 1024 segments per
    # workgroup: two windows
    assert len(_starts(SIZES[1], "fine")) - 1 < LDS_SEGS < len(_starts(SIZES[2], "coarse")) - 1
    assert -(-(SIZES[2] // 4) // 257) == 1022 and 1022 % 132 != 0
    assert (N_ONES // 4) // 64 == 2 * LDS_SEGS
    gaps = _starts(SIZES[1], "gaps")
    assert gaps[0] > 0 and gaps[-1] < SIZES[1] // 4 and bool(np.any(np.diff(gaps) == 0))


@pytest.mark.parametrize("n,kind", TABLES)
def test_every_segment_is_exact_in_absmax_and_within_the_fp64_bound_in_sumsq(n, kind):
    p, g = K._inputs(n)[:2]
    g0, p0 = g.clone(), p.clone()
    rig = Rig(n, kind).launch(g, p, index=5)
    _check(rig.result(), _input_reference(n, kind), rig.starts, (n, kind))
    assert rig.state.tolist() == [1, 1, 5, 0]
    # the launch only reads its inputs
    assert torch.equal(g.view(torch.int32), g0.view(torch.int32)) and torch.equal(p.view(torch.int32), p0.view(torch.int32))
    # a due word that is set changes nothing
    due = torch.tensor([1], dtype=torch.int32, device=dev())
    again = Rig(n, kind).launch(g, p, index=5, due=due)
    _check(again.result(), _input_reference(n, kind), rig.starts, (n, kind, "due"))


def _full(starts):
    """the segments that hold something, spread over the table"""
    full = np.flatnonzero(np.diff(starts) > 0)
    return [int(full[(len(full) - 1) * k // 5]) for k in range(6)]


@pytest.mark.parametrize("n,kind", TABLES[1:])
def test_squares_past_float32_range_and_below_it_are_kept(n, kind):
    """1e25 squared overflows fp32, 1e-30 squared underflows it to 0, 1e-40 is a float32 denormal: three segments of g and
    three others of p hold them"""
    starts = _starts(n, kind)
    segs = _full(starts)
    g_np, p_np = (x.copy() for x in _inputs_np(n))
    where = {"g": dict(zip((1e25, 1e-30, 1e-40), segs[:3])), "p": dict(zip((1e25, 1e-30, 1e-40), segs[3:]))}
    assert len(set(segs)) == 6
    for arr, key in ((g_np, "g"), (p_np, "p")):
        for value, s in where[key].items():
            arr[4 * starts[s]:4 * starts[s + 1]] = np.float32(value)
    assert np.float32(1e-40) != 0 and np.float32(1e-40) < np.finfo(np.float32).tiny
    rig = Rig(n, kind).launch(torch.from_numpy(g_np).to(dev()), torch.from_numpy(p_np).to(dev()), index=1)
    sumsq, absmax = rig.result()
    _check((sumsq, absmax), (_reference(g_np, starts), _reference(p_np, starts)), starts, (n, kind, "range"))
    for x, key in enumerate("gp"):
        for value, s in where[key].items():
            count = 4 * (starts[s + 1] - starts[s])
            got, want = float(sumsq[x, s]), count * float(np.float32(value)) ** 2
            assert np.isfinite(got) and got > 0, (key, value, got)
            assert abs(got - want) <= count * 2.0 ** -52 * want, (key, value, got, want)
            assert abs(got - count * value * value) <= 1e-4 * count * value * value, (key, value, got)
            assert absmax[x, s] == np.float32(value).view(np.uint32), (key, value)


@pytest.mark.parametrize("n,kind", TABLES[1:])
def test_inf_and_nan_show_in_their_segments_and_in_no_other(n, kind):
    starts = _starts(n, kind)
    segs = _full(starts)
    g_np, p_np = (x.copy() for x in _inputs_np(n))
    nan_bits = {"g": 0xffc12345, "p": 0x7f800001}  # a negative quiet NaN with a payload; the smallest signalling one
    where = {"g": (segs[0], segs[5]), "p": (segs[4], segs[2])}  # (segment of the inf, segment of the NaN)
    for arr, key in ((g_np, "g"), (p_np, "p")):
        s_inf, s_nan = where[key]
        arr[4 * starts[s_inf + 1] - 1] = -np.inf  # the last element of the segment
        arr.view(np.uint32)[4 * starts[s_nan]] = nan_bits[key]  # the first
    rig = Rig(n, kind).launch(torch.from_numpy(g_np).to(dev()), torch.from_numpy(p_np).to(dev()), index=1)
    sumsq, absmax = rig.result()
    # (the generic check holds every other segment to the reference, which is finite there)
    _check((sumsq, absmax), (_reference(g_np, starts), _reference(p_np, starts)), starts, (n, kind, "non-finite"))
    for x, key in enumerate("gp"):
        s_inf, s_nan = where[key]
        assert sumsq[x, s_inf] == np.inf and absmax[x, s_inf] == 0x7f800000, key
        assert np.isnan(sumsq[x, s_nan]) and absmax[x, s_nan] == nan_bits[key] & 0x7fffffff, key
        assert int(np.sum(~np.isfinite(sumsq[x]))) == 2, key


@pytest.mark.parametrize("n,kind", TABLES)
def test_three_samples_in_a_row_do_not_leak_into_each_other(n, kind):
    starts = _starts(n, kind)
    g_np, p_np = _inputs_np(n)
    rig = Rig(n, kind)
    for k, (scale, shift) in enumerate(((1.0, 0), (1e-3, 1), (40.0, 7)), start=1):
        gk, pk = np.roll(g_np, shift) * np.float32(scale), np.roll(p_np, 2 * shift) * np.float32(1.0 / scale)
        rig.launch(torch.from_numpy(gk).to(dev()), torch.from_numpy(pk).to(dev()), index=10 + k)
        _check(rig.result(), (_reference(gk, starts), _reference(pk, starts)), starts, (n, kind, "sample %d" % k))
        assert rig.state.tolist() == [1, k, 10 + k, 0]


@pytest.mark.parametrize("n,kind", TABLES)
def test_a_launch_that_does_not_sample_writes_nothing(n, kind):
    p, g = K._inputs(n)[:2]
    zero = torch.tensor([0], dtype=torch.int32, device=dev())
    one = torch.tensor([1], dtype=torch.int32, device=dev())
    for every, index, due in ((1, 1, zero), (3, 4, None), (3, 5, one), (0, 0, None), (0, 3, one)):
        rig = Rig(n, kind, every=every, fill=0x5a5a5a5a)
        before = rig.words()
        rig.launch(g, p, index=index, due=due)
        for a, b in zip(rig.words(), before):
            assert torch.equal(a, b), (every, index, due)
    # and the multiple of the interval is taken
    rig = Rig(n, kind, every=3, fill=0x5a5a5a5a).launch(g, p, index=6, due=one)
    assert rig.state.tolist() == [3, 0x5a5a5a5a + 1, 6, 0x5a5a5a5a]
    _check(rig.result(), _input_reference(n, kind), rig.starts, (n, kind, "every 3"))


def test_bad_arguments_are_rejected_before_the_launch():
    from mesm_amd import _lib
    n = SIZES[1]
    p, g = K._inputs(n)[:2]
    rig = Rig(n, "fine", fill=0x5a5a5a5a)
    before = rig.words()
    idx = torch.tensor([1], dtype=torch.int32, device=dev())
    a = lambda t: t.data_ptr()
    good = dict(g=a(g), p=a(p), n=n, seg=a(rig.table), n_seg=rig.n_seg, due=None, index=a(idx), st=a(rig.state),
                sumsq=a(rig.sumsq), absmax=a(rig.absmax))

    def call(**over):
        c = dict(good, **over)
        return _lib.lib().mesm_tensor_stats(c["g"], c["p"], c["n"], c["seg"], c["n_seg"], c["due"], c["index"], c["st"],
                                            c["sumsq"], c["absmax"], _lib.stream_ptr())

    for name in ("g", "p", "seg", "index", "st", "sumsq", "absmax"):
        assert call(**{name: None}) == EINVAL, name
    for over in (dict(n=0), dict(n=-4), dict(n=n + 2), dict(n=4 * (1 << 31)), dict(n_seg=0),
                 dict(n_seg=_lib.GUARD_MAX_SEGMENTS + 1)):
        assert call(**over) == EINVAL, over
    for name in ("g", "p"):
        assert call(**{name: good[name] + 4}) == EALIGN and call(**{name: good[name] + 8}) == EALIGN, name
    for name in ("seg", "index", "st", "absmax"):
        assert call(**{name: good[name] + 2}) == EALIGN, name
    assert call(due=good["index"] + 2) == EALIGN and call(sumsq=good["sumsq"] + 4) == EALIGN
    torch.cuda.synchronize()
    for x, y in zip(rig.words(), before):
        assert torch.equal(x, y)
