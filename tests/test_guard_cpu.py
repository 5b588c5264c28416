"""The non-finite guard of the flat AdamW (mesm_amd/optim.py: skip_nonfinite=) as far as it goes without a device: the
argument checks of mesm_grad_guard (include/mesm_gfx950.h), the mirror of MesmGuardState, the segment table of a gradient
buffer whose packs permute the offsets, and the switch in build_optimizer."""
import argparse
import ctypes

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


def test_state_mirror_is_four_words():
    from mesm_amd import _lib
    assert ctypes.sizeof(_lib.GuardState) == 16
    assert [n for n, _ in _lib.GuardState._fields_] == ["attempts", "skipped", "consecutive", "last_skipped_attempt"]
    assert _lib.GUARD_MAX_SEGMENTS >= 1024


def test_bad_arguments_are_rejected_without_a_gpu():
    """every call below fails a check in front of the launch (the addresses are never followed)"""
    from mesm_amd import _lib
    L = _lib.lib()
    A = 0x10000  # 16-byte aligned
    good = dict(g=A, n=64, seg=A + 0x100, n_seg=3, partials=A + 0x200, np=1, due=None, step=A + 0x300, gs=A + 0x310,
                go=A + 0x320, norm=A + 0x330, elems=A + 0x340)

    def call(**over):
        a = dict(good, **over)
        return L.mesm_grad_guard(a["g"], a["n"], a["seg"], a["n_seg"], a["partials"], a["np"], a["due"], a["step"], a["gs"],
                                 a["go"], a["norm"], a["elems"], None)

    for name in ("g", "seg", "partials", "step", "gs", "go", "elems"):
        assert call(**{name: None}) == EINVAL, name
    for over in (dict(n=0), dict(n=-4), dict(n=66), dict(n=4 * (1 << 31)), dict(n_seg=0),
                 dict(n_seg=_lib.GUARD_MAX_SEGMENTS + 1), dict(np=0), dict(np=1025)):
        assert call(**over) == EINVAL, over
    assert call(g=A + 4) == EALIGN and call(g=A + 8) == EALIGN
    for name in ("seg", "due", "step", "gs", "go", "norm"):
        assert call(**{name: A + 0x402}) == EALIGN, name
    assert call(elems=A + 0x404) == EALIGN


def test_segment_limit_is_reported_in_words():
    from mesm_amd import _lib
    from mesm_amd.optim import check_guard_segments
    check_guard_segments(1)
    check_guard_segments(_lib.GUARD_MAX_SEGMENTS)
    for n in (0, _lib.GUARD_MAX_SEGMENTS + 1):
        with pytest.raises(_lib.MesmError, match="segments, and the gradient buffer holds %d tensors" % n):
            check_guard_segments(n)


def _check_table(gb):
    from mesm_amd.optim import segment_table
    starts, order = segment_table(gb)
    assert starts.dtype == torch.int32 and len(starts) == len(gb.params) + 1 and sorted(order) == list(range(len(gb.params)))
    s = starts.tolist()
    assert s[0] == 0 and s[-1] == gb.numel // 4 and gb.numel % 4 == 0
    assert all(a < b for a, b in zip(s, s[1:]))  # sorted, no empty segment
    for j, i in enumerate(order):
        assert 4 * s[j] == gb.offsets[i], gb.names[i]                                    # gb.offsets, in float4s
        assert 4 * s[j + 1] == gb.offsets[i] + (gb.params[i].numel() + 3) // 4 * 4, gb.names[i]  # no gap up to the next
    return s, order


def test_segment_table_of_a_buffer_with_a_pack():
    from mesm_amd.gradbuf import GradBuffer
    mk = lambda *shape: torch.nn.Parameter(torch.zeros(*shape))
    named = [("a.weight", mk(8, 4)), ("odd", mk(5)), ("b.weight", mk(8, 4)), ("one", mk(1)), ("c.weight", mk(4, 4)),
             ("tail", mk(3, 3))]
    gb = GradBuffer(named, packs={"abc": ["a.weight", "b.weight", "c.weight"]})
    assert gb.offsets != sorted(gb.offsets)  # the pack pulled b.weight and c.weight in front of `odd`
    s, order = _check_table(gb)
    assert [gb.names[i] for i in order] == ["a.weight", "b.weight", "c.weight", "odd", "one", "tail"]
    assert s == [0, 8, 16, 20, 22, 23, 26]  # 5, 1 and 9 elements are padded to 8, 4 and 12


def test_segment_table_of_the_model():
    gb = _model().gradbuf()
    assert gb.packs and gb.offsets != sorted(gb.offsets)
    _check_table(gb)


def test_build_optimizer_honours_the_flag():
    from mesm_amd.optim import FlatAdamW, build_optimizer
    ns = argparse.Namespace(lr=1e-3, weight_decay=1e-2, lr_drop=100, gamma=0.1)
    opt = build_optimizer(ns, _model())[0]  # the reference's namespace has no such switch
    assert opt.skip_nonfinite is False and opt.guard_tensors() == []
    ns.skip_nonfinite = True
    assert build_optimizer(ns, _model())[0].skip_nonfinite is True
    assert FlatAdamW(_model(), lr=1e-3).skip_nonfinite is False
    with pytest.raises(RuntimeError, match="without skip_nonfinite"):
        FlatAdamW(_model(), lr=1e-3).nonfinite_report()
