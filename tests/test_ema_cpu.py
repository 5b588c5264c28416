"""The weight EMA of the flat AdamW (mesm_amd/optim.py: ema_decay=) as far as it goes without a device: the host mirror of
the kernels' decay schedule against the closed form, what the constructor refuses, and the argument checks of the five new C
entry points (include/mesm_gfx950.h: mesm_adamw_step_ema, ..._ema_gated, ..._groups_ema, ..._groups_ema_gated,
mesm_swap_f32)."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import ema_ref
from golden_io import Fixture

_FX = Fixture("qvh_tiny")


def _model():
    args = argparse.Namespace(**_FX.cfg)
    args.device = "cpu"
    from mesm_amd import build_model
    torch.manual_seed(3)
    return build_model(args)


@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("n", [0, 1, 9, 999])
def test_decay_schedule_against_the_closed_form(n, warmup):
    """(1 + n) and (10 + n) are exact in float32 for these n, the quotient is rounded once and the minimum is exact: the
    mirror is within half a unit in the last place, a relative 2^-24, of the closed form"""
    from mesm_amd.optim import ema_decay_at
    for decay in (0.999, 0.9999, 0.5, 0.05):
        got = ema_decay_at(n, decay, warmup)
        want = ema_ref.decay_schedule(n, decay, warmup)
        assert isinstance(got, np.float32)
        assert abs(float(got) - want) <= 2.0 ** -24 * want, (n, decay, warmup, float(got), want)
        if not warmup:
            assert got == np.float32(decay)
    if warmup:  # the values a reader can check by hand
        assert ema_decay_at(0, 0.999, True) == np.float32(0.1)
        assert ema_decay_at(1, 0.999, True) == np.float32(2.0) / np.float32(11.0)
        assert ema_decay_at(9, 0.999, True) == np.float32(10.0) / np.float32(19.0)
        assert ema_decay_at(999, 0.999, True) == np.float32(1000.0) / np.float32(1009.0)
        assert ema_decay_at(999, 0.99, True) == np.float32(0.99)


def test_reference_recurrence_is_the_formula():
    e0 = np.array([1.0, -2.0, 0.5], dtype=np.float32)
    p = [np.array([0.0, -2.0, 1.5], dtype=np.float32), np.array([1.0, -2.0, 2.5], dtype=np.float32)]
    e, big = ema_ref.ema_recurrence(e0, p, [np.float32(0.5), np.float32(0.25)])
    assert np.array_equal(e, np.array([0.25 * 0.5 + 0.75, -2.0, 0.25 * 1.0 + 0.75 * 2.5]))
    assert np.array_equal(big, np.array([1.0, 2.0, 2.5]))
    kept, _ = ema_ref.ema_recurrence(e0, p, [np.float32(0.5)] * 2, written=np.array([True, False, False]))
    assert np.array_equal(kept[1:], e0[1:].astype(np.float64))


def test_constructor_refusals_and_defaults():
    from mesm_amd.optim import FlatAdamW, build_optimizer
    model = _model()
    for bad in (0.0, 1.0, -0.1, 1.5, 1.0 - 1e-9):  # (the last one IS 1 as a float32: the average would never move)
        with pytest.raises(ValueError, match="ema_decay"):
            FlatAdamW(model, lr=1e-3, ema_decay=bad)
    off = FlatAdamW(model, lr=1e-3)
    assert off.ema_decay is None and off.ema is None and off.ema_tensors() == []
    for what in (off.reset_ema, off.ema_state_dict, lambda: off.swap_ema().__enter__(), lambda: off.num_updates):
        with pytest.raises(RuntimeError, match="without ema_decay"):
            what()
    with pytest.raises(RuntimeError, match="without ema_decay"):
        off.ema_decay = 0.9
    on = FlatAdamW(_model(), lr=1e-3, ema_decay=0.999, ema_warmup=True)
    assert on.ema_decay == 0.999 and on.ema_warmup is True
    on.ema_decay = 0.99
    assert on.ema_decay == 0.99
    with pytest.raises(ValueError, match="ema_decay"):
        on.ema_decay = 1.0
    assert on.ema_decay == 0.99
    # build_optimizer: the reference's namespace has neither switch; one that has them gets the EMA
    ns = argparse.Namespace(lr=1e-3, weight_decay=1e-2, lr_drop=100, gamma=0.1)
    assert build_optimizer(ns, _model())[0].ema_decay is None
    ns.ema_decay, ns.ema_warmup = 0.9995, True
    opt = build_optimizer(ns, _model())[0]
    assert opt.ema_decay == 0.9995 and opt.ema_warmup is True


def test_ema_state_struct_is_16_bytes():
    from mesm_amd import _lib
    assert ctypes.sizeof(_lib.EmaState) == 16
    assert (_lib.EmaState.decay.offset, _lib.EmaState.warmup.offset, _lib.EmaState.step0.offset) == (0, 4, 8)


EINVAL, EALIGN = -1, -2


def _default_call(L, gated, **kw):
    a = dict(p=0x1000, g=0x2000, m=0x3000, v=0x4000, active4=None, n=64, partials=None, np=0, max_norm=0.0, lr=0x5000,
             step=0x7000, norm_out=None, due=0x7100, ema=0x8000, es=0x9000, decay_out=None)
    a.update(kw)
    head = (a["p"], a["g"], a["m"], a["v"], a["active4"], a["n"], a["partials"], a["np"], a["max_norm"], a["lr"], 0.9, 0.999,
            1e-8, 1e-2, a["step"], a["norm_out"])
    tail = (a["ema"], a["es"], a["decay_out"], None)
    if gated:
        return L.mesm_adamw_step_ema_gated(*head, a["due"], *tail)
    return L.mesm_adamw_step_ema(*head, *tail)


def _groups_call(L, gated, **kw):
    a = dict(p=0x1000, g=0x2000, m=0x3000, v=0x4000, tag4=0x5001, n=64, partials=None, np=0, max_norm=0.0, groups=0x6000,
             n_groups=3, step=0x7000, norm_out=None, due=0x7100, ema=0x8000, es=0x9000, decay_out=None)
    a.update(kw)
    head = (a["p"], a["g"], a["m"], a["v"], a["tag4"], a["n"], a["partials"], a["np"], a["max_norm"], a["groups"],
            a["n_groups"], a["step"], a["norm_out"])
    tail = (a["ema"], a["es"], a["decay_out"], None)
    if gated:
        return L.mesm_adamw_step_groups_ema_gated(*head, a["due"], *tail)
    return L.mesm_adamw_step_groups_ema(*head, *tail)


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("call", [_default_call, _groups_call])
def test_ema_entries_reject_bad_arguments_without_a_gpu(call, gated):
    from mesm_amd import _lib
    L = _lib.lib()
    # what the EMA adds
    assert call(L, gated, ema=None) == EINVAL
    assert call(L, gated, es=None) == EINVAL
    assert call(L, gated, ema=None, es=None) == EINVAL
    for off in (4, 8, 12):
        assert call(L, gated, ema=0x8000 + off) == EALIGN, off
    assert call(L, gated, ema=0x8004, es=None) == EINVAL  # what is invalid AND misaligned is invalid
    # the twin's own checks are still there
    for name in ("p", "g", "m", "v", "step"):
        assert call(L, gated, **{name: None}) == EINVAL, name
    for n in (0, -4, 6):
        assert call(L, gated, n=n) == EINVAL, n
    assert call(L, gated, max_norm=0.1) == EINVAL  # clipping without partials
    assert call(L, gated, max_norm=0.1, partials=0x8000, np=1025) == EINVAL
    for name in ("p", "g", "m", "v"):
        assert call(L, gated, **{name: 0x1000 + 4}) == EALIGN, name
    if gated:
        assert call(L, gated, due=None) == EINVAL
        assert call(L, gated, due=0x7102) == EINVAL
    if call is _groups_call:
        for name in ("tag4", "groups"):
            assert call(L, gated, **{name: None}) == EINVAL, name
        for n_groups in (0, 65):
            assert call(L, gated, n_groups=n_groups) == EINVAL, n_groups
    else:
        assert call(L, gated, lr=None) == EINVAL


def test_swap_rejects_bad_arguments_without_a_gpu():
    from mesm_amd import _lib
    L = _lib.lib()
    assert L.mesm_swap_f32(None, 0x2000, 64, None) == EINVAL
    assert L.mesm_swap_f32(0x1000, None, 64, None) == EINVAL
    for n in (0, -4, 6):
        assert L.mesm_swap_f32(0x1000, 0x2000, n, None) == EINVAL, n
    assert L.mesm_swap_f32(0x1004, 0x2000, 64, None) == EALIGN
    assert L.mesm_swap_f32(0x1000, 0x2008, 64, None) == EALIGN
    assert L.mesm_swap_f32(0x1004, 0x2000, 6, None) == EINVAL
