"""The weight EMA inside the AdamW launches (include/mesm_gfx950.h: mesm_adamw_step_ema, mesm_adamw_step_ema_gated,
mesm_adamw_step_groups_ema, mesm_adamw_step_groups_ema_gated) and mesm_swap_f32, through direct ctypes calls.

p, m, v, the norm and the step count must be the twin entry's bits; the average of every element the update writes must be
within 4 * 2^-24 * max(|e_old|, |p_new|) of the fp64 formula (tests/ema_ref.py) fed the device's own p_new and decay -- the
expression has two roundings, an analytic bound of 3 such units -- and every element the update skips keeps its bits.

Sizes: one float4; 3 * 256 + 5 float4 (a partly filled last workgroup); 262144 + 300 float4 (past the 1024-workgroup cap:
the grid-stride loop takes a second pass)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ema_ref

pytestmark = pytest.mark.gpu

SIZES = (4, 4 * (3 * 256 + 5), 4 * (262144 + 300))
SEGMENTS = (1, 1, 2, 16, 75, 37)  # run lengths in groups of 4 (132 in all): boundaries fall inside a wave
# (count the update sees, MesmEmaState.step0): n = 0, 999 and 9 earlier averages
STEPS = ((1, 0), (1000, 0), (1000, 990))
DECAY = 0.999


def dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """(p, g, m, v, e) with gradient magnitudes log-uniform in 1e-4..1 and an average that sits from 1e-6 to 1 away from
    the parameter; never modified (the tests work on clones)"""
    gen = torch.Generator(device=dev()).manual_seed(11 + n % 97)
    rnd = lambda f: f(n, device=dev(), generator=gen, dtype=torch.float32)
    p, m, v = rnd(torch.randn), 0.1 * rnd(torch.randn), 0.01 * rnd(torch.rand)
    mag = torch.pow(10.0, -4.0 * rnd(torch.rand))
    g = torch.where(rnd(torch.rand) < 0.5, -mag, mag)
    e = p + torch.pow(10.0, -6.0 * rnd(torch.rand)) * rnd(torch.randn)
    return p, g, m, v, e


@functools.lru_cache(maxsize=None)
def _mask(n):
    """active bytes: random at p = 0.5, plus a run of ones and a run of zeros that start and end off 64-lane boundaries"""
    n4 = n // 4
    gen = torch.Generator().manual_seed(3)
    mask = (torch.rand(n4, generator=gen) < 0.5).to(torch.uint8)
    if n4 > 700:
        mask[37:37 + 100] = 1   # lanes 37 .. 136
        mask[203:203 + 77] = 0  # lanes 203 .. 279: across the first workgroup's end
        mask[n4 - 3:] = 1       # the partly filled last workgroup writes
    else:
        mask[:] = 1
    return mask.to(dev())


@functools.lru_cache(maxsize=None)
def _tags(n):
    """three groups in runs whose borders fall inside a wave, zeroed where _mask is 0"""
    n4 = n // 4
    lens = torch.tensor(SEGMENTS * (n4 // sum(SEGMENTS) + 1))
    vals = torch.tensor([1 + j % 3 for j in range(len(lens))], dtype=torch.uint8)
    tags = torch.repeat_interleave(vals, lens)[:n4].contiguous().to(dev())
    return tags * _mask(n)


def _table(t):
    """three groups; the third joined at the current count (step0 == step): it is not live yet"""
    from mesm_amd import _lib
    rows = ((1e-3, (0.9, 0.999), 1e-8, 1e-2, 0), (1e-4, (0.8, 0.99), 1e-6, 0.0, min(2, t - 1)), (1e-3, (0.9, 0.999), 1e-8, 0.1, t))
    arr = (_lib.AdamGroup * len(rows))()
    for r, (lr, (b1, b2), eps, wd, step0) in zip(arr, rows):
        r.lr, r.beta1, r.beta2, r.eps, r.weight_decay, r.step0 = lr, b1, b2, eps, wd, step0
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev())


def _ema_state(decay, warmup, step0):
    from mesm_amd import _lib
    st = _lib.EmaState(decay=decay, warmup=int(warmup), step0=step0, reserved=0)
    return torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8).to(dev())


def _written(form, n, t):
    """per element: the update writes it"""
    if form == "default":
        w4 = _mask(n) != 0
    else:
        tags = _tags(n)
        w4 = (tags == 1) | (tags == 2)  # tag 3: the group that is not live; tag 0: skipped
    return torch.repeat_interleave(w4, 4)


def _update(form, n, t, clip, ema=None, due=None, lr=1e-3, wd=1e-2, inputs=None):
    """one (clip +) update on fresh copies of the inputs through the entry that `ema` (None, or (decay, warmup, step0)) and
    `due` (None, or the device word) select -> every buffer the launches may write"""
    from mesm_amd._lib import check, lib, ptr, stream_ptr
    L = lib()
    p, g, m, v, e = (x.clone() for x in (inputs or _inputs(n)))
    norm = torch.full((1,), -1.0, device=dev(), dtype=torch.float32)
    dout = torch.full((1,), -1.0, device=dev(), dtype=torch.float32)
    partials, n_p = None, 0
    if clip:  # the sum of squares advances the count
        step_t = torch.tensor([t - 1], dtype=torch.int32, device=dev())
        partials = torch.full((1024,), -7.0, device=dev(), dtype=torch.float32)
        c_np = ctypes.c_int32(0)
        if due is None:
            check(L.mesm_grad_sumsq(ptr(g), n, ptr(partials), ctypes.byref(c_np), ptr(step_t), stream_ptr()), "sumsq")
        else:
            check(L.mesm_grad_sumsq_gated(ptr(g), n, ptr(partials), ctypes.byref(c_np), ptr(step_t), ptr(due), stream_ptr()),
                  "sumsq gated")
        n_p = c_np.value
    else:
        step_t = torch.tensor([t], dtype=torch.int32, device=dev())
    max_norm = 0.1 if clip else 0.0
    if form == "groups":
        table = _table(t)
        head = (ptr(p), ptr(g), ptr(m), ptr(v), ptr(_tags(n)), n, ptr(partials), n_p, max_norm, ptr(table), 3, ptr(step_t),
                ptr(norm))
        name = "mesm_adamw_step_groups"
    else:
        lr_t = torch.full((1,), lr, device=dev())
        head = (ptr(p), ptr(g), ptr(m), ptr(v), ptr(_mask(n)), n, ptr(partials), n_p, max_norm, ptr(lr_t), 0.9, 0.999, 1e-8,
                wd, ptr(step_t), ptr(norm))
        name = "mesm_adamw_step"
    tail = ()
    if ema is not None:
        es = _ema_state(*ema)
        name, tail = name + "_ema", (ptr(e), ptr(es), ptr(dout))
    if due is not None:
        name, head = name + "_gated", head + (ptr(due),)
    check(getattr(L, name)(*head, *tail, stream_ptr()), name)
    torch.cuda.synchronize()
    return dict(p=p, m=m, v=v, step=step_t, norm=norm, ema=e, decay_out=dout)


def test_masks_and_sizes_are_where_the_kernel_can_go_wrong():
    assert SIZES[0] == 4 and (SIZES[1] // 4) % 256 == 5 and SIZES[2] // 4 == 1024 * 256 + 300
    for n in SIZES[1:]:
        mask = _mask(n).long().cpu()
        assert 0.4 < float(mask.float().mean()) < 0.6
        assert bool(mask[37:137].all()) and not bool(mask[203:280].any()) and 37 % 64 and 137 % 64 and 203 % 64 and 280 % 64
        tags = _tags(n).long().cpu()
        starts = torch.nonzero(tags[1:] != tags[:-1]).flatten() + 1
        assert bool((starts % 64 != 0).any()) and set(tags.tolist()) == {0, 1, 2, 3}
    assert _mask(4).tolist() == [1] and _tags(4).tolist() == [1]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form", ["default", "groups"])
def test_update_with_ema_against_the_twin_entry_and_float64(form, n):
    from mesm_amd.optim import ema_decay_at
    e_old = _inputs(n)[4]
    worst_units, worst_ulp = 0.0, 0.0
    for t, step0 in STEPS:
        written = _written(form, n, t)
        assert bool(written.any())
        for warmup in (False, True):
            for clip in (False, True):
                what = (form, n, t, step0, warmup, clip)
                ref = _update(form, n, t, clip)
                got = _update(form, n, t, clip, ema=(DECAY, warmup, step0))
                due = torch.tensor([1], dtype=torch.int32, device=dev())
                gated = _update(form, n, t, clip, ema=(DECAY, warmup, step0), due=due)
                for name in ("p", "m", "v", "step", "norm"):  # the twin's bits
                    assert torch.equal(_bits(got[name]), _bits(ref[name])), (what, name)
                for name in got:  # the gated entry on a due replay: the ungated one's bits, the average included
                    assert torch.equal(_bits(gated[name]), _bits(got[name])), (what, name)
                assert int(got["step"]) == t and (float(got["norm"]) > 0) == clip  # (-1: never written)
                assert not torch.equal(got["p"][written], _inputs(n)[0][written])
                # the decay: within one unit in the last place of the host mirror
                d_dev = np.float32(got["decay_out"].item())
                d_host = ema_decay_at(t - 1 - step0, DECAY, warmup)
                ulp = abs(float(d_dev) - float(d_host)) / float(np.spacing(d_host))
                worst_ulp = max(worst_ulp, ulp)
                assert ulp <= 1.0, (what, float(d_dev), float(d_host))
                assert abs(float(d_host) - ema_ref.decay_schedule(t - 1 - step0, DECAY, warmup)) <= 2.0 ** -24
                # written elements: the fp64 formula on the device's p_new and decay
                w = written.cpu().numpy()
                eo, pn, en = (x.cpu().numpy() for x in (e_old, got["p"], got["ema"]))
                want = ema_ref.ema_update(eo[w], pn[w], d_dev)
                unit = ema_ref.EMA_UNIT * np.maximum(np.abs(eo[w].astype(np.float64)), np.abs(pn[w].astype(np.float64)))
                units = float(np.max(np.abs(en[w].astype(np.float64) - want) / unit))
                worst_units = max(worst_units, units)
                assert units <= ema_ref.EMA_UNITS, (what, units)
                assert bool(np.any(en[w] != eo[w]))
                # skipped elements keep their bits
                assert torch.equal(_bits(got["ema"][~written]), _bits(e_old[~written])), what
    print("%s, n = %d: worst EMA error %.3f units of 2^-24 * max(|e_old|, |p_new|) (bound %d), decay_out %.2f ulp from "
          "ema_decay_at" % (form, n, worst_units, ema_ref.EMA_UNITS, worst_ulp))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form", ["default", "groups"])
def test_a_gated_launch_that_is_not_due_touches_nothing(form, n):
    due = torch.tensor([0], dtype=torch.int32, device=dev())
    got = _update(form, n, 1000, True, ema=(DECAY, True, 0), due=due)
    p, g, m, v, e = _inputs(n)
    for name, t in (("p", p), ("m", m), ("v", v), ("ema", e)):
        assert torch.equal(_bits(got[name]), _bits(t)), name
    assert int(got["step"]) == 999 and float(got["norm"]) == -1.0 and float(got["decay_out"]) == -1.0


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", ["lr=0", "wd=0"])
def test_an_average_equal_to_the_parameter_is_a_fixed_point(case, n):
    """e == p, zero gradient and zero moments: with lr = 0 or weight_decay = 0 the update leaves p as it is, and
    fmaf(d, e - p, p) = fmaf(d, 0, p) = p exactly"""
    p = _inputs(n)[0]
    zero = torch.zeros_like(p)
    lr, wd = (0.0, 1e-2) if case == "lr=0" else (1e-3, 0.0)
    for warmup in (False, True):
        got = _update("default", n, 5, False, ema=(DECAY, warmup, 0), lr=lr, wd=wd, inputs=(p, zero, zero, zero, p))
        assert torch.equal(_bits(got["p"]), _bits(p))
        assert torch.equal(_bits(got["ema"]), _bits(got["p"]))
        assert float(got["decay_out"]) > 0


@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_bits_and_twice_is_the_identity(n):
    from mesm_amd._lib import check, lib, ptr, stream_ptr
    a0, b0 = _inputs(n)[0], _inputs(n)[4]
    # (with bit patterns that are no ordinary numbers: the exchange moves bits, it does no arithmetic)
    a0 = a0.clone()
    a0[:4] = torch.tensor([float("nan"), float("inf"), -0.0, 1e-42], device=dev())
    a, b = a0.clone(), b0.clone()
    check(lib().mesm_swap_f32(ptr(a), ptr(b), n, stream_ptr()), "mesm_swap_f32")
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(b0)) and torch.equal(_bits(b), _bits(a0))
    check(lib().mesm_swap_f32(ptr(a), ptr(b), n, stream_ptr()), "mesm_swap_f32")
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(a0)) and torch.equal(_bits(b), _bits(b0))
    check(lib().mesm_swap_f32(ptr(a), ptr(a), n, stream_ptr()), "mesm_swap_f32")  # a buffer with itself: nothing to do
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(a0))
