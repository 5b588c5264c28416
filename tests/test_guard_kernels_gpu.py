"""mesm_grad_guard (include/mesm_gfx950.h) between the sum of squares and the gated AdamW entries, through direct ctypes
calls: inputs, masks, tags, group table and sizes are those of tests/test_ema_kernels_gpu.py.

Every comparison is on bits or integers.  A finite gradient must give, through sum of squares -> guard -> gated update on the
guard's word, what sum of squares -> ungated update gives; a gradient with inf / NaN in it, or one whose sum of squares
overflows, must leave every buffer and the step count alone, count the elements per segment exactly, and leave the next
finite update bit-equal to one that never saw it.

Segment tables: run lengths (1, 1, 2, 16, 75, 37) float4 repeated ("fine": borders inside a wave; 11 931 segments at the
largest size, past the 2048 that sit in LDS, so the table is searched in global memory) and, at the largest size only, the
same lengths times 16 ("coarse": 746 segments, the LDS path with the grid-stride loop in its fifth pass)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import test_ema_kernels_gpu as K

pytestmark = pytest.mark.gpu

SIZES, SEGMENTS = K.SIZES, K.SEGMENTS
TABLES = [(n, "fine") for n in SIZES] + [(SIZES[2], "coarse")]
FORMS = [("default", False), ("default", True), ("groups", False), ("groups", True)]  # (update form, with EMA)
T = 1000                  # the count a successful update sees
EMA = (0.999, True, 990)  # warm-up under way: the decay depends on the count, so a count left wrong shows in the average
CLIP = 0.1
LDS_SEGS = 2048           # csrc/optim.hip: GUARD_LDS_SEGS
dev, _bits = K.dev, K._bits


@functools.lru_cache(maxsize=None)
def _starts(n, kind):
    """float4 starts of the segments plus the end, as a numpy int64 array"""
    n4 = n // 4
    scale = 16 if kind == "coarse" else 1
    lens = np.array(SEGMENTS * (n4 // (scale * sum(SEGMENTS)) + 1), dtype=np.int64) * scale
    s = np.concatenate([[0], np.cumsum(lens)])
    s = s[s < n4]
    return np.concatenate([s, [n4]])


@functools.lru_cache(maxsize=None)
def _table(n, kind):
    return torch.tensor(_starts(n, kind), dtype=torch.int32).to(dev())


def _expected(n, kind, elements):
    """per segment: how many of the element indices fall into it"""
    s = _starts(n, kind)
    seg = np.searchsorted(s, np.asarray(elements, dtype=np.int64) // 4, side="right") - 1
    return np.bincount(seg, minlength=len(s) - 1).astype(np.int64)


class Rig:
    """one optimizer state on the device plus everything the three launches write"""

    def __init__(self, form, ema, n, kind, clip=True, go=7):
        p, _, m, v, e = K._inputs(n)
        self.form, self.ema, self.n, self.clip = form, ema, n, clip
        self.p, self.m, self.v, self.e = p.clone(), m.clone(), v.clone(), e.clone()
        i32 = lambda *x: torch.tensor(x, dtype=torch.int32, device=dev())
        self.step, self.go, self.gs = i32(T - 1), i32(go), i32(0, 0, 0, 0)
        self.norm = torch.full((1,), -1.0, device=dev())
        self.dout = torch.full((1,), -1.0, device=dev())
        self.partials = torch.full((1024,), -7.0, device=dev())
        self.table = _table(n, kind)
        self.n_seg = len(self.table) - 1
        self.elems = torch.zeros(self.n_seg, dtype=torch.int64, device=dev())
        self.groups = K._table(T)
        self.lr = torch.full((1,), 1e-3, device=dev())
        self.es = K._ema_state(*EMA)

    def _sumsq(self, g, due):
        from mesm_amd._lib import check, lib, ptr, stream_ptr
        c_np = ctypes.c_int32(0)
        if due is None:
            check(lib().mesm_grad_sumsq(ptr(g), self.n, ptr(self.partials), ctypes.byref(c_np), ptr(self.step), stream_ptr()),
                  "sumsq")
        else:
            check(lib().mesm_grad_sumsq_gated(ptr(g), self.n, ptr(self.partials), ctypes.byref(c_np), ptr(self.step), ptr(due),
                                              stream_ptr()), "sumsq gated")
        return c_np.value

    def _update(self, g, n_p, due):
        from mesm_amd._lib import check, lib, ptr, stream_ptr
        max_norm = CLIP if self.clip else 0.0
        head = (ptr(self.p), ptr(g), ptr(self.m), ptr(self.v))
        if self.form == "groups":
            name = "mesm_adamw_step_groups"
            head += (ptr(K._tags(self.n)), self.n, ptr(self.partials), n_p, max_norm, ptr(self.groups), 3, ptr(self.step),
                     ptr(self.norm))
        else:
            name = "mesm_adamw_step"
            head += (ptr(K._mask(self.n)), self.n, ptr(self.partials), n_p, max_norm, ptr(self.lr), 0.9, 0.999, 1e-8, 1e-2,
                     ptr(self.step), ptr(self.norm))
        tail = ()
        if self.ema:
            name, tail = name + "_ema", (ptr(self.e), ptr(self.es), ptr(self.dout))
        if due is not None:
            name, head = name + "_gated", head + (ptr(due),)
        check(getattr(lib(), name)(*head, *tail, stream_ptr()), name)

    def plain(self, g):
        """sum of squares, ungated update: what the optimizer does without the guard"""
        self._update(g, self._sumsq(g, None), None)
        torch.cuda.synchronize()
        return self

    def guarded(self, g, due=None):
        """sum of squares, guard, the gated twin of the update on the guard's word"""
        from mesm_amd._lib import check, lib, ptr, stream_ptr
        n_p = self._sumsq(g, due)
        check(lib().mesm_grad_guard(ptr(g), self.n, ptr(self.table), self.n_seg, ptr(self.partials), n_p, ptr(due),
                                    ptr(self.step), ptr(self.gs), ptr(self.go), ptr(self.norm), ptr(self.elems), stream_ptr()),
              "mesm_grad_guard")
        self._update(g, n_p, self.go)
        torch.cuda.synchronize()
        return self

    def buffers(self):
        return dict(p=self.p, m=self.m, v=self.v, ema=self.e, decay_out=self.dout)

    def snapshot(self):
        return {k: t.clone() for k, t in self.buffers().items()}

    def same_buffers(self, other, what):
        for name, t in self.buffers().items():
            assert torch.equal(_bits(t), _bits(other[name])), (what, name)


@functools.lru_cache(maxsize=None)
def _reference(form, ema, n, clip=True):
    """the unguarded update of the fresh state with the finite gradient; never modified"""
    rig = Rig(form, ema, n, "fine", clip).plain(K._inputs(n)[1])
    return dict(rig.snapshot(), step=rig.step.clone(), norm=rig.norm.clone())


def test_tables_are_where_the_kernel_can_go_wrong():
    for n, kind in TABLES:
        s = _starts(n, kind)
        assert s[0] == 0 and s[-1] == n // 4 and bool(np.all(np.diff(s) > 0))
    assert len(_starts(SIZES[0], "fine")) - 1 == 1
    assert 1 < len(_starts(SIZES[1], "fine")) - 1 <= LDS_SEGS and bool(np.any(_starts(SIZES[1], "fine") % 64 != 0))
    assert len(_starts(SIZES[2], "fine")) - 1 > LDS_SEGS >= len(_starts(SIZES[2], "coarse")) - 1 > 256
    assert SIZES[2] // 4 > 4 * 256 * 256  # the guard's 256 workgroups of 256 lanes go round more than four times
    assert _expected(SIZES[1], "fine", [0, 3, 4, 8, 4 * 20 - 1, 4 * 20]).tolist()[:5] == [2, 1, 1, 1, 1]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form,ema", FORMS)
def test_finite_gradients_give_the_unguarded_update(form, ema, n):
    g = K._inputs(n)[1]
    for clip in (True, False):
        ref = _reference(form, ema, n, clip)
        rig = Rig(form, ema, n, "fine", clip).guarded(g)
        rig.same_buffers(ref, (form, ema, n, clip))
        assert not torch.equal(rig.p, K._inputs(n)[0])
        assert int(rig.step) == int(ref["step"]) == T and int(rig.go) == 1
        assert rig.gs.tolist() == [1, 0, 0, 0] and int(rig.elems.abs().sum()) == 0
        if clip:
            assert torch.equal(_bits(rig.norm), _bits(ref["norm"]))
        else:  # (the unclipped update writes no norm; the guard does: the clipped run's, from the same partials)
            assert float(ref["norm"]) == -1.0
            assert torch.equal(_bits(rig.norm), _bits(_reference(form, ema, n, True)["norm"]))
        assert bool(torch.isfinite(rig.norm)) and float(rig.norm) > 0
        # a due word that is set changes nothing
        due = torch.tensor([1], dtype=torch.int32, device=dev())
        gated = Rig(form, ema, n, "fine", clip).guarded(g, due=due)
        gated.same_buffers(ref, (form, ema, n, clip, "due"))
        assert int(gated.step) == T and int(gated.go) == 1 and gated.gs.tolist() == [1, 0, 0, 0]


def _poison_cases(n, kind):
    """[(label, element indices)]: single elements at the places the issue names, three segments at once, everything"""
    s = _starts(n, kind)
    n_seg = len(s) - 1
    k = min(4, n_seg - 1)  # a segment border inside a wave (float4 20 of the fine table)
    single = {"first": 0, "last": n - 1, "end of a segment": 4 * int(s[k + 1]) - 1, "start of the next": 4 * int(s[k + 1]),
              "past float4 262144": 4 * 262144 + 1}
    cases = [(label, [e]) for label, e in single.items() if 0 <= e < n]
    three = sorted({0, min(4, n_seg - 1), n_seg - 1})
    cases.append(("segments %s" % three, np.concatenate([np.arange(4 * s[j], 4 * s[j + 1]) for j in three])))
    return cases


def _skip_then_recover(form, ema, n, kind, g_bad, expected, what):
    """the checks every poisoned gradient must pass"""
    good = K._inputs(n)[1]
    rig = Rig(form, ema, n, kind)
    before = rig.snapshot()
    for attempt in (1, 2):
        rig.guarded(g_bad)
        rig.same_buffers(before, (what, attempt))
        assert int(rig.step) == T - 1 and int(rig.go) == 0, (what, attempt)
        assert rig.gs.tolist() == [attempt] * 4, (what, attempt, rig.gs.tolist())
        assert not bool(torch.isfinite(rig.norm)), (what, attempt, float(rig.norm))
        assert np.array_equal(rig.elems.cpu().numpy(), attempt * expected), (what, attempt)
    rig.guarded(good)  # the next finite gradient: as if the bad ones had never been seen
    ref = _reference(form, ema, n)
    rig.same_buffers(ref, (what, "recover"))
    assert int(rig.step) == T and int(rig.go) == 1 and rig.gs.tolist() == [3, 2, 0, 2], (what, rig.gs.tolist())
    assert torch.equal(_bits(rig.norm), _bits(ref["norm"])), what
    assert np.array_equal(rig.elems.cpu().numpy(), 2 * expected), what


@pytest.mark.parametrize("n,kind", TABLES)
@pytest.mark.parametrize("form,ema", FORMS)
def test_poisoned_elements_skip_the_update_and_are_counted(form, ema, n, kind):
    good = K._inputs(n)[1]
    for label, elements in _poison_cases(n, kind):
        expected = _expected(n, kind, elements)
        assert int(expected.sum()) == len(elements)
        idx = torch.as_tensor(np.asarray(elements, dtype=np.int64), device=dev())
        for value in (float("inf"), float("-inf"), float("nan")):
            g_bad = good.clone()
            g_bad[idx] = value
            _skip_then_recover(form, ema, n, kind, g_bad, expected, (form, ema, n, kind, label, value))


@pytest.mark.parametrize("n,kind", TABLES)
def test_a_buffer_that_is_nan_throughout(n, kind):
    g_bad = torch.full((n,), float("nan"), device=dev())
    expected = 4 * np.diff(_starts(n, kind))
    assert int(expected.sum()) == n
    for form, ema in FORMS:
        _skip_then_recover(form, ema, n, kind, g_bad, expected, (form, ema, n, kind, "all NaN"))


@pytest.mark.parametrize("n,kind", TABLES)
def test_a_launch_that_is_not_due_writes_go_and_nothing_else(n, kind):
    g_bad = K._inputs(n)[1].clone()
    g_bad[n - 1] = float("inf")
    due = torch.tensor([0], dtype=torch.int32, device=dev())
    for form, ema in FORMS:
        for go in (1, 0):
            rig = Rig(form, ema, n, kind, go=go)
            before = rig.snapshot()
            rig.guarded(g_bad, due=due)
            rig.same_buffers(before, (form, ema, go))
            assert int(rig.go) == 0 and rig.gs.tolist() == [0, 0, 0, 0] and int(rig.elems.abs().sum()) == 0
            assert int(rig.step) == T - 1 and float(rig.norm) == -1.0
            assert bool((rig.partials == -7.0).all())


@pytest.mark.parametrize("n,kind", TABLES)
def test_an_overflowing_sum_of_squares_skips_and_counts_nothing(n, kind):
    """every element a finite 1.5e19: one square is 2.25e38, the four of a float4 together are past float32"""
    g_big = torch.full((n,), 1.5e19, device=dev())
    assert bool(torch.isfinite(g_big).all()) and bool(torch.isfinite(g_big * g_big).all())
    for form, ema in FORMS:
        rig = Rig(form, ema, n, kind)
        before = rig.snapshot()
        rig.guarded(g_big)
        rig.same_buffers(before, (form, ema))
        assert int(rig.go) == 0 and rig.gs.tolist() == [1, 1, 1, 1] and int(rig.step) == T - 1
        assert float(rig.norm) == float("inf")
        assert int(rig.elems.abs().sum()) == 0
