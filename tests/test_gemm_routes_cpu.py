"""The routing of the GEMM calls, pinned on the CPU: mesm_gemm_plan (plan without launch) must reproduce, field for field,
what the dispatch code did before the one-plan refactor for every call of tests/gemm_route_cases.py under every
(MESM_GEMM_BF16X, MESM_GEMM_TILE) pair -- tests/gemm_routes.json was recorded from THAT code, its launch sites patched to
record the kernel instantiation instead of launching -- and the forced-kernel switch must do what the forced-kernel GPU
tests say it does."""
import ctypes
import json
import os

import pytest

import gemm_route_cases as rc
from mesm_amd import _lib
from mesm_amd.testing import gemm_forced

HERE = os.path.dirname(os.path.abspath(__file__))
TILE32, TILE64, TILE128, FRAG, WSTAGE, WSTAGE64, WTALL, LDS64 = range(8)


def plan(problems, grouped):
    """[(position, family, variant, launch)] per problem, in the call's order"""
    arr, n = rc.make_args(problems)
    out = (ctypes.c_int32 * (4 * n))()
    _lib.check(_lib.lib().mesm_gemm_plan(arr, n if grouped else 0, out), "mesm_gemm_plan")
    return [tuple(out[4 * i:4 * i + 4]) for i in range(n)]


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(HERE, "gemm_routes.json")) as f:
        return json.load(f)


def test_the_record_covers_the_list(recorded):
    calls = rc.calls()
    assert recorded["calls"] == [name for name, _, _ in calls]
    assert set(recorded["routes"]) == {"%d,%d" % (b, t) for b in rc.SWITCH_BF16X for t in rc.SWITCH_TILE}
    for col in recorded["routes"].values():
        assert len(col) == len(calls)


@pytest.mark.parametrize("bf16x", rc.SWITCH_BF16X)
@pytest.mark.parametrize("tile", rc.SWITCH_TILE)
def test_plan_reproduces_the_recorded_routes(recorded, bf16x, tile):
    L = _lib.lib()
    tile0, bf0 = L.mesm_gemm_get_force_tile(), L.mesm_gemm_get_bf16x()
    col = recorded["routes"]["%d,%d" % (bf16x, tile)]
    wrong = []
    try:
        _lib.check(L.mesm_gemm_set_switches(tile, bf16x), "mesm_gemm_set_switches")
        for (name, grouped, problems), idx in zip(rc.calls(), col):
            want = recorded["plans"][idx]
            got = [x for row in plan(problems, grouped) for x in row]
            if got != want:
                wrong.append((name, got, want))
    finally:
        L.mesm_gemm_set_switches(tile0, bf0)
    assert not wrong, "%d calls routed differently, first: %r" % (len(wrong), wrong[:3])
    assert (L.mesm_gemm_get_force_tile(), L.mesm_gemm_get_bf16x()) == (tile0, bf0)


def test_every_kernel_form_of_the_record_is_reached(recorded):
    """the (family, variant) pairs the recorded code launched somewhere in the list all appear in the plans"""
    seen = {(p[i + 1], p[i + 2]) for p in recorded["plans"] for i in range(0, len(p), 4)}
    assert seen == {tuple(v) for v in recorded["kernels"].values()}
    assert len(seen) >= 50


def family(p, grouped=False):
    return plan([p], grouped)[0][1]


PLAIN = rc.P(2400, 256, 256, bt=True)


def test_the_force_switch_forces():
    """what the forced-kernel tests of tests/test_kernels_gpu.py rely on"""
    with gemm_forced(0):
        auto = family(PLAIN)
    assert auto != LDS64
    with gemm_forced(3):
        assert family(PLAIN) == LDS64
    with gemm_forced(1):  # frag_ok: 16-byte aligned operands, K % 4 == 0
        assert family(PLAIN) == FRAG
        assert family(rc.P(2400, 256, 258, bt=True)) != FRAG  # K % 4: refused, the automatic register-staged tile
    with gemm_forced(2):
        assert family(PLAIN) == WSTAGE
        assert family(rc.P(2400, 256, 256, bt=True, A2=True)) in (TILE32, TILE64, TILE128)  # no addends on LDS-DMA
    with gemm_forced(4):
        assert family(PLAIN) == WSTAGE64
    with gemm_forced(6):
        assert family(PLAIN) == WTALL
        # wtall has no colsum output: refused, and the launch falls through to the automatic choice (for this shape, 152
        # tiles of 64 x 64, the 32 x 32 register-staged tile)
        assert family(rc.P(2400, 256, 256, bt=True, colsum=True)) == TILE32
        assert family(rc.P(8192, 1024, 256, bt=True, colsum=True)) == TILE128
    for tile, fam in ((32, TILE32), (64, TILE64), (128, TILE128)):
        with gemm_forced(tile):
            assert family(PLAIN) == fam
    with gemm_forced(128):
        assert family(rc.P(2400, 256, 256, bt=True, B2=True)) != TILE128  # the 128 tile has no addend form
    with gemm_forced(64):
        assert family(rc.P(2400, 256, 256, bt=True, B2=True)) == TILE64


def test_gemm_forced_restores_what_was_in_force():
    L = _lib.lib()
    before = (L.mesm_gemm_get_force_tile(), L.mesm_gemm_get_bf16x())
    with gemm_forced(3):
        assert L.mesm_gemm_get_force_tile() == 3
        with gemm_forced(1):
            assert L.mesm_gemm_get_force_tile() == 1
        assert L.mesm_gemm_get_force_tile() == 3
    with pytest.raises(ZeroDivisionError):
        with gemm_forced(4):
            1 / 0
    assert (L.mesm_gemm_get_force_tile(), L.mesm_gemm_get_bf16x()) == before


def test_plan_rejects_what_the_launch_rejects():
    L = _lib.lib()
    out = (ctypes.c_int32 * 8)()
    g = _lib.GemmArgs()
    assert L.mesm_gemm_plan(ctypes.byref(g), 0, out) == -1  # MESM_EINVAL: null operands
    assert L.mesm_gemm_plan(ctypes.byref(g), 1, out) == -1
    assert L.mesm_gemm_plan(None, 1, out) == -1
    arr, n = rc.make_args([PLAIN])
    assert L.mesm_gemm_plan(arr, 1, None) == -1
    assert L.mesm_gemm_plan(arr, 65, out) == -1
