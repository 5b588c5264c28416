"""FlatAdamW(tensor_stats=k) on qvh_tiny weights (mesm_amd/optim.py, mesm_tensor_stats): eager steps, sampling, the non-finite
guard in front of it, the captured micro-stepped tail, and the switch left off.  Model, batch, twins and optimizer forms are
those of tests/test_ema_gpu.py; the inf goes into a gradient view behind a clean backward as in tests/test_guard_gpu.py.

Bounds.  absmax is exact.  A tensor's sum of squares is a sum of n exact, non-negative fp64 terms: the device's and the
reference's each err by at most (n - 1) * 2^-53 relative, and the two square roots add 2^-53 each, so the norms differ by at
most (n + 1) * 2^-53 relative; the tests allow n * 2^-52 like the kernel tests do on the sums.  `total_grad_norm` against
`last_norm`: the fp32 path behind last_norm is about 70 dependent additions deep, 70 * 2^-24 = 4.2e-6 on the square, half of
that on the root: 1e-5 relative."""
import argparse

import numpy as np
import pytest
import torch

import test_ema_gpu as E

pytestmark = pytest.mark.gpu

CLIP = 0.1
dev, _same = E.dev, E._same


def _expected(model, flat_g, flat_p):
    """{name: (grad_norm, grad_absmax, param_norm, param_absmax, elements)} from copies of the two flat buffers, in fp64"""
    gb = model.gradbuf()
    g, p = flat_g.detach().cpu().numpy(), flat_p.detach().cpu().numpy()
    out = {}
    for name, q, off in zip(gb.names, gb.params, gb.offsets):
        sl = slice(off, off + q.numel())
        with np.errstate(over="ignore", invalid="ignore"):
            out[name] = (float(np.sqrt(np.sum(g[sl].astype(np.float64) ** 2))), float(np.abs(g[sl]).max()),
                         float(np.sqrt(np.sum(p[sl].astype(np.float64) ** 2))), float(np.abs(p[sl]).max()), q.numel())
    return out


def _close(got, want, n):
    if not np.isfinite(want):
        return (np.isnan(got) and np.isnan(want)) or got == want
    return abs(got - want) <= n * 2.0 ** -52 * want


def _check_report(rep, want, what, grad=True, param=True):
    assert set(rep["tensors"]) == set(want), what
    for name, (gn, gm, pn, pm, n) in want.items():
        t = rep["tensors"][name]
        if grad:
            assert _close(t["grad_norm"], gn, n), (what, name, t["grad_norm"], gn)
            assert t["grad_absmax"] == gm or (np.isnan(gm) and np.isnan(t["grad_absmax"])), (what, name)
        if param:
            assert _close(t["param_norm"], pn, n), (what, name, t["param_norm"], pn)
            assert t["param_absmax"] == pm, (what, name)


def _stat_words(opt):
    return [t.clone() for t in opt.tensor_stat_tensors()]


@pytest.mark.parametrize("clip", [CLIP, 0.0])
@pytest.mark.parametrize("form", ["default", "groups"])
def test_eager_step_reports_the_gradient_it_saw_and_the_parameters_before_it(form, clip, deterministic_forward):
    model, crit = E._model()
    twin, _ = E._model()
    opt = E._make_opt(model, form, tensor_stats=1)
    opt_t = E._make_opt(twin, form)
    gb = model.gradbuf()
    assert opt.tensor_stats_every == 1 and len(opt.tensor_stat_tensors()) == 3 and opt_t.tensor_stat_tensors() == []
    empty = opt.tensor_stats()
    assert empty["samples"] == 0 and empty["tensors"] == {}
    E._backward(model, crit)
    p_before = opt.flat_p.clone()
    opt.step(grad_clip=clip)
    E._twin_step(twin, opt_t, model, clip=clip)
    torch.cuda.synchronize()
    rep = opt.tensor_stats()
    assert rep["samples"] == 1 and rep["attempt"] == 1
    want = _expected(model, gb.flat, p_before)
    _check_report(rep, want, (form, clip))
    for name, q in zip(gb.names, gb.params):  # the gradient statistics are those of p.grad
        assert rep["tensors"][name]["has_grad"] == (q.grad is not None), name
        if q.grad is not None:
            assert _close(rep["tensors"][name]["grad_norm"], float(q.grad.double().norm()), q.numel()), name
            assert rep["tensors"][name]["grad_absmax"] == float(q.grad.abs().max()), name
    assert any(t["has_grad"] for t in rep["tensors"].values()) and rep["total_grad_norm"] > 0
    total = float(np.sqrt(sum(v[0] ** 2 for v in want.values())))
    assert abs(rep["total_grad_norm"] - total) <= 1e-12 * total
    if clip:
        assert abs(rep["total_grad_norm"] - float(opt.last_norm)) <= 1e-5 * float(opt.last_norm)
    # per group: the root of its tensors' sums
    assert len(rep["groups"]) == len(opt.param_groups)
    for k, grp in enumerate(rep["groups"]):
        mine = [want[gb.names[i]] for i in range(len(gb.params)) if opt._group_of[i] == k]
        for key, col in (("grad_norm", 0), ("param_norm", 2)):
            ref = float(np.sqrt(sum(v[col] ** 2 for v in mine)))
            assert abs(grp[key] - ref) <= 1e-12 * ref, (k, key)
    # the twin without the switch ends with the same bits
    assert not _same(opt.flat_p, p_before)
    for a, b in ((opt.flat_p, opt_t.flat_p), (opt.exp_avg, opt_t.exp_avg), (opt.exp_avg_sq, opt_t.exp_avg_sq),
                 (opt.step_t, opt_t.step_t)):
        assert _same(a, b)
    assert _same(opt.last_norm, opt_t.last_norm) if clip else (opt.last_norm is None and opt_t.last_norm is None)


def test_every_second_attempt_is_sampled_and_an_edit_takes_effect_at_the_next_step(deterministic_forward):
    model, crit = E._model()
    opt = E._make_opt(model, "default", tensor_stats=2)
    E._backward(model, crit)
    seen = []
    for _ in range(4):
        opt.step(grad_clip=CLIP)
        rep = opt.tensor_stats()
        seen.append((rep["samples"], rep["attempt"]))
    assert seen == [(0, 0), (1, 2), (1, 2), (2, 4)]
    opt.tensor_stats_every = 1
    p_before = opt.flat_p.clone()
    opt.step(grad_clip=CLIP)
    rep = opt.tensor_stats()
    assert (rep["samples"], rep["attempt"]) == (3, 5)
    _check_report(rep, _expected(model, model.gradbuf().flat, p_before), "every 1")
    opt.tensor_stats_every = 0  # paused
    words = _stat_words(opt)
    opt.step(grad_clip=CLIP)
    torch.cuda.synchronize()
    assert int(opt._stats_state[0]) == 0
    for a, b in zip(_stat_words(opt)[1:], words[1:]):
        assert torch.equal(a, b)
    assert torch.equal(opt._stats_state[1:], words[0][1:])
    for bad in (-1, 1.5, "2", True):
        with pytest.raises(ValueError, match="tensor_stats"):
            opt.tensor_stats_every = bad


@pytest.mark.parametrize("form", ["default", "groups"])
def test_behind_the_guard_a_skipped_attempt_is_sampled_and_the_next_is_its_own(form, deterministic_forward):
    model, crit = E._model()
    opt = E._make_opt(model, form, skip_nonfinite=True, tensor_stats=1)
    gb = model.gradbuf()
    i = next(i for i, p in enumerate(gb.params) if p is E._left_out(model))
    name, off = gb.names[i], gb.offsets[i]
    E._backward(model, crit)
    opt.step(grad_clip=CLIP)
    assert opt.tensor_stats()["samples"] == 1
    # a clean backward, then an inf in one element of the weight's gradient view
    E._backward(model, crit)
    view = dict(model.named_parameters())[name].grad
    assert view.data_ptr() == gb.flat.data_ptr() + 4 * off
    view.view(-1)[7] = float("inf")
    p_before = opt.flat_p.clone()
    opt.step(grad_clip=CLIP)
    torch.cuda.synchronize()
    assert _same(opt.flat_p, p_before) and opt.skipped_updates == 1 and int(opt.step_t) == 1
    rep = opt.tensor_stats()
    assert (rep["samples"], rep["attempt"]) == (2, 2)
    assert rep["tensors"][name]["grad_norm"] == float("inf") and rep["tensors"][name]["grad_absmax"] == float("inf")
    bad = {n for n, t in rep["tensors"].items() if not np.isfinite(t["grad_norm"])}
    assert bad == set(opt.nonfinite_report()["elements"]) == {name}
    assert rep["total_grad_norm"] == float("inf")
    _check_report(rep, _expected(model, gb.flat, p_before), (form, "skipped"))
    # the next clean step: the step count repeats (2 again), the attempt does not
    E._backward(model, crit)
    p_before = opt.flat_p.clone()
    opt.step(grad_clip=CLIP)
    torch.cuda.synchronize()
    assert int(opt.step_t) == 2 and not _same(opt.flat_p, p_before)
    rep = opt.tensor_stats()
    assert (rep["samples"], rep["attempt"]) == (3, 3)
    _check_report(rep, _expected(model, gb.flat, p_before), (form, "recovered"))
    assert all(np.isfinite(t["grad_norm"]) for t in rep["tensors"].values())
    # finite elements whose squares overflow fp32: the guard can only say norm_overflow, the statistics name the tensor
    E._backward(model, crit)
    opt.nonfinite_report()
    view = dict(model.named_parameters())[name].grad
    view.fill_(1e25)
    p_before = opt.flat_p.clone()
    opt.step(grad_clip=CLIP)
    torch.cuda.synchronize()
    assert _same(opt.flat_p, p_before)
    assert opt.nonfinite_report()["since_last_report"] == {"skipped": 1, "elements": {}, "norm_overflow": True}
    rep = opt.tensor_stats()
    assert (rep["samples"], rep["attempt"]) == (4, 4)
    huge = {n for n, t in rep["tensors"].items() if t["grad_norm"] > 1e19}
    assert huge == {name}
    got, want = rep["tensors"][name]["grad_norm"], float(np.float32(1e25)) * float(np.sqrt(view.numel()))
    assert np.isfinite(got) and abs(got - want) <= view.numel() * 2.0 ** -52 * want
    assert np.isfinite(rep["total_grad_norm"]) and rep["total_grad_norm"] >= got
    _check_report(rep, _expected(model, gb.flat, p_before), (form, "overflow"))


@pytest.mark.parametrize("form", ["default", "groups"])
def test_captured_tail_samples_the_due_replays_and_no_other(form, deterministic_forward):
    from mesm_amd.graphed import StepCache
    model, crit = E._model()
    opt = E._make_opt(model, form, tensor_stats=1)
    cache = StepCache(model, crit, "qvhighlights", micro_steps=2, optimizer=opt, grad_clip=CLIP)
    items = E._shards()
    gb = model.gradbuf()

    def replay(i):
        cache.run(items[i][0], draws=items[i][1])
        torch.cuda.synchronize()

    def due_replay(samples, attempt):
        p_before = opt.flat_p.clone()
        replay(1)
        assert cache.update_due and not _same(opt.flat_p, p_before)
        rep = opt.tensor_stats()
        assert (rep["samples"], rep["attempt"]) == (samples, attempt)
        _check_report(rep, _expected(model, gb.flat, p_before), (form, "due replay", attempt))
        assert all(rep["tensors"][n]["has_grad"] == bool(on) for n, on in zip(gb.names, cache._cycle.covered))

    fresh = _stat_words(opt)
    assert fresh[0].tolist() == [1, 0, 0, 0]
    # the first replay of a cycle is not due; its graph was captured just now, warm-up passes included: no sample
    replay(0)
    assert not cache.update_due
    for a, b in zip(_stat_words(opt), fresh):
        assert torch.equal(a, b)
    assert opt.tensor_stats()["samples"] == 0
    due_replay(1, 1)  # (the second shard's graph is captured here: its warm-up passes leave no sample either)
    assert cache.captures == 2
    after = _stat_words(opt)
    replay(0)
    for a, b in zip(_stat_words(opt), after):
        assert torch.equal(a, b)
    due_replay(2, 2)  # four replays, two samples
    # an edit of the interval is followed without a new capture
    opt.tensor_stats_every = 2
    after = _stat_words(opt)
    replay(0)
    replay(1)
    assert cache.update_due and int(opt.step_t) == 3
    now = _stat_words(opt)
    assert now[0].tolist() == [2, 2, 2, 0] and torch.equal(now[1], after[1]) and torch.equal(now[2], after[2])
    replay(0)
    due_replay(3, 4)
    assert cache.captures == 2 and len(opt.captured_ptrs()) == 16


def test_without_the_switch_nothing_of_it_exists(deterministic_forward):
    from mesm_amd.optim import FlatAdamW, build_optimizer
    model, crit = E._model()
    opt = FlatAdamW(model)
    assert opt.tensor_stat_tensors() == [] and opt.tensor_stats_every is None and len(opt.captured_ptrs()) == 12
    assert all(getattr(opt, a) is None for a in ("_stats_state", "_stats_sumsq", "_stats_absmax", "_stats_table"))
    with pytest.raises(RuntimeError, match="without tensor_stats"):
        opt.tensor_stats()
    with pytest.raises(RuntimeError, match="without tensor_stats"):
        opt.tensor_stats_every = 3
    fx = E._fx()
    ns = argparse.Namespace(lr=1e-3, weight_decay=1e-2, lr_drop=10, gamma=0.1, tensor_stats=7)
    model2, _ = E._model()
    on = build_optimizer(ns, model2)[0]
    assert on.tensor_stats_every == 7 and int(on._stats_state[0]) == 7 and len(on.captured_ptrs()) == 16
    assert "tensor_stats" not in on.state_dict() and set(on.state_dict()) == {"state", "param_groups"}
    assert fx is not None
