"""Per-tensor statistics of the flat AdamW (mesm_amd/optim.py: tensor_stats=) as far as they go without a device: the
report assembled from raw arrays, the host's sum over the workgroups' slots, the argument checks of mesm_tensor_stats
(include/mesm_gfx950.h), the mirror of MesmStatsState, the constructor's refusals and the switch in build_optimizer."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

from golden_io import Fixture

_FX = Fixture("qvh_tiny")
EINVAL, EALIGN = -1, -2


def _model():
    args = argparse.Namespace(**_FX.cfg)
    args.device = "cpu"
    from mesm_amd import build_model
    torch.manual_seed(3)
    return build_model(args)


def _bits(x):
    return np.array(x, dtype=np.float32).view(np.uint32)


def test_state_mirror_is_four_words():
    from mesm_amd import _lib
    assert ctypes.sizeof(_lib.StatsState) == 16
    assert [n for n, _ in _lib.StatsState._fields_] == ["every", "samples", "last_attempt", "reserved"]


def test_report_follows_the_segment_order_and_sums_the_groups():
    from mesm_amd.optim import tensor_stats_report
    names = ["a.weight", "a.bias", "b.weight", "frozen"]
    order = [2, 0, 3, 1]         # segment j holds parameter order[j]: a pack moved b.weight to the front
    group_of = [0, 1, 0, -1]     # weights, biases, and a tensor no group covers
    has_grad = [True, True, False, True]
    sumsq = np.array([[9.0, 16.0, 4.0, 1.0], [25.0, 144.0, 0.0, 1e-80]])  # per SEGMENT: gradient row, parameter row
    absmax = np.stack([_bits([3.0, 2.5, np.inf, 1.0]), _bits([5.0, 12.0, 0.0, 1e-40])])
    rep = tensor_stats_report(names, order, group_of, 2, has_grad, 37, 3700, sumsq, absmax)
    assert rep["samples"] == 37 and rep["attempt"] == 3700 and list(rep["tensors"]) == ["b.weight", "a.weight", "frozen", "a.bias"]
    assert rep["tensors"]["b.weight"] == {"grad_norm": 3.0, "grad_absmax": 3.0, "param_norm": 5.0, "param_absmax": 5.0,
                                          "has_grad": False}
    assert rep["tensors"]["a.weight"] == {"grad_norm": 4.0, "grad_absmax": 2.5, "param_norm": 12.0, "param_absmax": 12.0,
                                          "has_grad": True}
    assert rep["tensors"]["frozen"]["grad_absmax"] == float("inf") and rep["tensors"]["frozen"]["param_norm"] == 0.0
    assert rep["tensors"]["a.bias"]["param_norm"] == pytest.approx(1e-40, rel=1e-15)
    assert rep["tensors"]["a.bias"]["param_absmax"] == float(np.float32(1e-40))
    assert rep["total_grad_norm"] == float(np.sqrt(30.0))  # every segment, covered or not
    assert rep["groups"][0] == {"grad_norm": 5.0, "param_norm": 13.0} and rep["groups"][1]["grad_norm"] == 1.0
    assert rep["groups"][1]["param_norm"] == pytest.approx(1e-40, rel=1e-15) and len(rep["groups"]) == 2
    # non-finite sums come through as they are, in their tensor, its group and the total
    sumsq[0, 1] = np.inf
    sumsq[1, 3] = np.nan
    absmax[1, 3] = 0x7fc00001
    rep = tensor_stats_report(names, order, group_of, 2, has_grad, 1, 1, sumsq, absmax)
    assert rep["tensors"]["a.weight"]["grad_norm"] == float("inf") and rep["tensors"]["b.weight"]["grad_norm"] == 3.0
    assert np.isnan(rep["tensors"]["a.bias"]["param_norm"]) and np.isnan(rep["tensors"]["a.bias"]["param_absmax"])
    assert rep["groups"][0]["grad_norm"] == float("inf") and np.isnan(rep["groups"][1]["param_norm"])
    assert rep["groups"][1]["grad_norm"] == 1.0 and rep["total_grad_norm"] == float("inf")


def test_report_before_the_first_sample_is_empty():
    from mesm_amd.optim import tensor_stats_report
    rep = tensor_stats_report(["w"], [0], [0], 1, None, 0, 0, None, None)
    assert rep == {"samples": 0, "attempt": 0, "total_grad_norm": None, "tensors": {}, "groups": []}


def test_slots_of_a_segment_are_added_over_the_workgroups_that_meet_it():
    """3 workgroups of 4 float4 over 10 float4; segments [1, 1) (empty), [1, 5), [5, 6), [6, 10): slot = segment + workgroup"""
    from mesm_amd.optim import reduce_stat_slots
    starts, n4, n_wg = [1, 1, 5, 6, 10], 10, 3
    n_slots = 4 + 3
    nan = np.nan  # a slot no (workgroup, segment) pair owns is never read
    g = [nan, 1.0, 2.0, 4.0, 8.0, 16.0, nan]  # seg 1: wg 0 (slot 1), wg 1 (slot 2); seg 2: wg 1 (slot 3); seg 3: wg 1, 2
    p = [nan, 0.5, 0.25, 3.0, 1.0, 1e300, nan]
    mg = [77, 5, 9, 2, 7, 3, 77]
    mp = [77, 1, 0, 0x7f800000, 4, 0x7fc00000, 77]
    sumsq, absmax = reduce_stat_slots(starts, n4, n_wg, np.array(g + p), np.array(mg + mp, dtype=np.uint32))
    assert sumsq.shape == absmax.shape == (2, 4) and len(g) == n_slots
    assert sumsq.tolist() == [[0.0, 3.0, 4.0, 24.0], [0.0, 0.75, 3.0, 1e300]]
    assert absmax.tolist() == [[0, 9, 2, 7], [0, 1, 0x7f800000, 0x7fc00000]]
    # one workgroup: slot = segment
    sumsq, absmax = reduce_stat_slots([0, 2, 3], 3, 1, np.array([1.0, 2.0, nan, 3.0, 4.0, nan]),
                                      np.array([1, 2, 77, 3, 4, 77], dtype=np.uint32))
    assert sumsq.tolist() == [[1.0, 2.0], [3.0, 4.0]] and absmax.tolist() == [[1, 2], [3, 4]]


def test_bad_arguments_are_rejected_without_a_gpu():
    """every call below fails a check in front of the launch (the addresses are never followed)"""
    from mesm_amd import _lib
    L = _lib.lib()
    A = 0x10000  # 16-byte aligned
    good = dict(g=A, p=A + 0x100, n=64, seg=A + 0x200, n_seg=3, due=None, index=A + 0x300, st=A + 0x310, sumsq=A + 0x320,
                absmax=A + 0x400)

    def call(**over):
        a = dict(good, **over)
        return L.mesm_tensor_stats(a["g"], a["p"], a["n"], a["seg"], a["n_seg"], a["due"], a["index"], a["st"], a["sumsq"],
                                   a["absmax"], None)

    for name in ("g", "p", "seg", "index", "st", "sumsq", "absmax"):
        assert call(**{name: None}) == EINVAL, name
    for over in (dict(n=0), dict(n=-4), dict(n=66), dict(n=4 * (1 << 31)), dict(n_seg=0),
                 dict(n_seg=_lib.GUARD_MAX_SEGMENTS + 1)):
        assert call(**over) == EINVAL, over
    for name in ("g", "p"):
        assert call(**{name: A + 4}) == EALIGN and call(**{name: A + 8}) == EALIGN, name
    for name in ("seg", "due", "index", "st", "absmax"):
        assert call(**{name: A + 0x502}) == EALIGN, name
    assert call(sumsq=A + 0x504) == EALIGN
    assert L.mesm_tensor_stats_workgroups(4) == 1 and L.mesm_tensor_stats_workgroups(4 * 1025) == 2
    assert L.mesm_tensor_stats_workgroups(4 * (1 << 30)) == 1024
    for n in (0, -4, 6, 4 * (1 << 31)):
        assert L.mesm_tensor_stats_workgroups(n) == EINVAL, n


def test_constructor_refuses_what_is_no_interval():
    from mesm_amd.optim import FlatAdamW
    model = _model()
    for bad in (0, -3, 2.0, "100", True, 1 << 31):
        with pytest.raises(ValueError, match="tensor_stats takes None or an int >= 1"):
            FlatAdamW(model, lr=1e-3, tensor_stats=bad)
    opt = FlatAdamW(model, lr=1e-3, tensor_stats=100)
    assert opt.tensor_stats_every == 100
    opt.tensor_stats_every = 0
    assert opt.tensor_stats_every == 0
    with pytest.raises(ValueError, match="tensor_stats"):
        opt.tensor_stats_every = -1
    off = FlatAdamW(_model(), lr=1e-3)
    assert off.tensor_stats_every is None and off.tensor_stat_tensors() == []
    with pytest.raises(RuntimeError, match="without tensor_stats"):
        off.tensor_stats()
    with pytest.raises(RuntimeError, match="without tensor_stats"):
        off.tensor_stats_every = 5


def test_segment_limit_is_reported_in_words():
    from mesm_amd import _lib
    from mesm_amd.optim import check_guard_segments
    what = "tensor_stats: mesm_tensor_stats reduces the tensors"
    check_guard_segments(_lib.GUARD_MAX_SEGMENTS, what)
    with pytest.raises(_lib.MesmError, match="tensor_stats: .* through a table of 1 to 65536 segments, and the gradient "
                                             "buffer holds 65537 tensors"):
        check_guard_segments(_lib.GUARD_MAX_SEGMENTS + 1, what)


def test_build_optimizer_reads_the_switch():
    from mesm_amd.optim import build_optimizer
    ns = argparse.Namespace(lr=1e-3, weight_decay=1e-2, lr_drop=10, gamma=0.1)
    opt, _ = build_optimizer(ns, _model())
    assert opt.tensor_stats_every is None and opt.tensor_stat_tensors() == []
    ns.tensor_stats = 50
    assert build_optimizer(ns, _model())[0].tensor_stats_every == 50
