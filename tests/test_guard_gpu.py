"""FlatAdamW(skip_nonfinite=True) on qvh_tiny weights (mesm_amd/optim.py, mesm_grad_guard): eager steps and the captured
micro-stepped update around one gradient with an inf in it, the report that names the tensor, checkpoints, and the switch
left off.  Model, batches, twins and optimizer forms are those of tests/test_ema_gpu.py and tests/test_micro_steps_gpu.py.

The poison only ever goes into the gradient buffer, behind a backward pass that was clean.  Every comparison is on bits or
integers: a twin optimizer WITHOUT the guard is fed clones of the clean gradients alone, and the guarded one must end with
its parameters, moments, average, step count and norm."""
import numpy as np
import pytest
import torch

import test_ema_gpu as E

pytestmark = pytest.mark.gpu

DECAY, CLIP = 0.999, 0.1
dev, _same = E.dev, E._same


def _state(opt):
    return [t.clone() for t in [opt.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.step_t] + opt.ema_tensors()]


def _guard_words(opt):
    return opt._guard_state.tolist(), int(opt._guard_go), int(opt._guard_counts.sum())


def _target(model):
    """(name, offset in the flat buffers) of a weight that every step writes a gradient for -- the tensor the grouped
    optimizers of these tests leave out: a non-finite gradient element skips the update wherever it sits"""
    gb = model.gradbuf()
    i = next(i for i, p in enumerate(gb.params) if p is E._left_out(model))
    return gb.names[i], gb.offsets[i]


def _has_grad(model):
    return [p.grad is not None for p in model.gradbuf().params]


def _same_optimizer(opt, ref, clip):
    for a, b in ((opt.flat_p, ref.flat_p), (opt.exp_avg, ref.exp_avg), (opt.exp_avg_sq, ref.exp_avg_sq), (opt.ema, ref.ema),
                 (opt.step_t, ref.step_t), (opt.last_ema_decay, ref.last_ema_decay)):
        if not _same(a, b):
            return False
    return _same(opt.last_norm, ref.last_norm) if clip else ref.last_norm is None


@pytest.mark.parametrize("clip", [CLIP, 0.0])
@pytest.mark.parametrize("form", ["default", "groups"])
def test_eager_step_over_an_inf_is_skipped_named_and_forgotten(form, clip, deterministic_forward):
    model, crit = E._model()
    twin, _ = E._model()
    opt = E._make_opt(model, form, ema_decay=DECAY, ema_warmup=True, skip_nonfinite=True)
    opt_t = E._make_opt(twin, form, ema_decay=DECAY, ema_warmup=True)
    gb = model.gradbuf()
    name, off = _target(model)
    assert opt.skipped_updates == 0 and len(opt.guard_tensors()) == 3 and opt_t.guard_tensors() == []
    # one clean step
    E._backward(model, crit)
    opt.step(grad_clip=clip)
    E._twin_step(twin, opt_t, model, clip=clip)
    torch.cuda.synchronize()
    assert _same_optimizer(opt, opt_t, clip) and opt.num_updates == 1 and bool(torch.isfinite(opt.last_norm))
    # a clean backward, then an inf in one element of the weight's gradient view
    E._backward(model, crit)
    view = dict(model.named_parameters())[name].grad
    assert view.data_ptr() == gb.flat.data_ptr() + 4 * off
    view.view(-1)[7] = float("inf")
    before = _state(opt)
    opt.step(grad_clip=clip)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(_state(opt), before)):  # parameters, moments, count, average, EMA words, last decay
        assert _same(a, b), i
    assert opt.num_updates == 1 and opt.skipped_updates == 1 and not bool(torch.isfinite(opt.last_norm))
    rep = opt.nonfinite_report()
    assert (rep["attempts"], rep["skipped"], rep["consecutive"], rep["last_skipped_attempt"]) == (2, 1, 1, 2)
    assert rep["elements"] == {name: 1}
    assert rep["since_last_report"] == {"skipped": 1, "elements": {name: 1}, "norm_overflow": False}
    again = opt.nonfinite_report()
    assert again["elements"] == {name: 1}
    assert again["since_last_report"] == {"skipped": 0, "elements": {}, "norm_overflow": False}
    # a further clean step: the twin took the two clean gradients only
    E._backward(model, crit)
    opt.step(grad_clip=clip)
    E._twin_step(twin, opt_t, model, clip=clip)
    torch.cuda.synchronize()
    assert _same_optimizer(opt, opt_t, clip) and opt.num_updates == 2 and int(opt.step_t) == 2
    assert not _same(opt.flat_p, before[0])
    rep = opt.nonfinite_report()
    assert (rep["attempts"], rep["skipped"], rep["consecutive"], rep["last_skipped_attempt"]) == (3, 1, 0, 2)
    # finite elements whose squares overflow: skipped, and reported as an overflow of the norm
    gb.flat.fill_(1.5e19)
    opt.step(grad_clip=clip)
    torch.cuda.synchronize()
    assert _same(opt.flat_p, opt_t.flat_p) and int(opt.step_t) == 2 and float(opt.last_norm) == float("inf")
    rep = opt.nonfinite_report()
    assert rep["since_last_report"] == {"skipped": 1, "elements": {}, "norm_overflow": True} and rep["elements"] == {name: 1}


@pytest.mark.parametrize("form", ["default", "groups"])
def test_captured_update_skips_the_cycle_with_the_inf_and_no_other(form, deterministic_forward):
    from mesm_amd.graphed import StepCache
    model, crit = E._model()
    twin, _ = E._model()
    opt = E._make_opt(model, form, ema_decay=DECAY, skip_nonfinite=True)
    opt_t = E._make_opt(twin, form, ema_decay=DECAY)
    cache = StepCache(model, crit, "qvhighlights", micro_steps=2, optimizer=opt, grad_clip=CLIP)
    items = E._shards()
    gb = model.gradbuf()
    name, off = _target(model)

    def replay(i):
        cache.run(items[i][0], draws=items[i][1])
        torch.cuda.synchronize()

    # cycle A, clean.  Its first replay captured a graph (warm-up passes and capture ran guarded updates) and is not due
    replay(0)
    assert not cache.update_due and _guard_words(opt) == ([0, 0, 0, 0], 0, 0)
    replay(1)
    assert cache.update_due and int(opt.step_t) == 1 and _guard_words(opt) == ([1, 0, 0, 0], 1, 0)
    E._twin_step(twin, opt_t, model)
    torch.cuda.synchronize()
    assert _same_optimizer(opt, opt_t, True)
    after_a = _state(opt)
    assert cache.captures == 2
    # cycle B: the host writes an inf between the two replays; the second accumulates on top of it
    replay(0)
    assert _guard_words(opt) == ([1, 0, 0, 0], 0, 0)  # a replay that is not due: the state as it was, go cleared
    gb.flat[off + 5] = float("inf")
    replay(1)
    assert cache.update_due
    for i, (a, b) in enumerate(zip(_state(opt), after_a)):
        assert _same(a, b), i
    assert not bool(torch.isfinite(opt.last_norm))  # (the poison survived the replay)
    assert opt.skipped_updates == 1 and opt.num_updates == 1 and _guard_words(opt) == ([2, 1, 1, 2], 0, 1)
    rep = opt.nonfinite_report()
    assert rep["since_last_report"] == {"skipped": 1, "elements": {name: 1}, "norm_overflow": False}
    # cycle C, clean: the second update, on the state cycle A left
    replay(0)
    assert _guard_words(opt) == ([2, 1, 1, 2], 0, 1)
    assert bool(torch.isfinite(gb.flat).all())  # the first replay of a cycle clears the buffer
    replay(1)
    assert cache.update_due and int(opt.step_t) == 2 and _guard_words(opt) == ([3, 1, 0, 2], 1, 1)
    E._twin_step(twin, opt_t, model)
    torch.cuda.synchronize()
    assert _same_optimizer(opt, opt_t, True) and opt.num_updates == 2
    assert not _same(opt.flat_p, after_a[0]) and cache.captures == 2
    assert opt.nonfinite_report()["since_last_report"] == {"skipped": 0, "elements": {}, "norm_overflow": False}


def test_state_dict_round_trip_and_torch_interchange(deterministic_forward):
    model, crit = E._model()
    opt = E._make_opt(model, "default", skip_nonfinite=True)
    gb = model.gradbuf()
    name, off = _target(model)
    E._backward(model, crit)
    opt.step(grad_clip=CLIP)
    g, has = gb.flat.clone(), _has_grad(model)
    gb.flat[off] = float("nan")
    opt.step(grad_clip=CLIP)
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups", "nonfinite"} and sd["nonfinite"] == {"skipped": 1, "attempts": 2}
    model2, _ = E._model()
    model2.load_state_dict(model.state_dict())
    opt2 = E._make_opt(model2, "default", skip_nonfinite=True)
    opt2.load_state_dict(sd)
    assert opt2.skipped_updates == 1 and int(opt2.step_t) == 1
    rep = opt2.nonfinite_report()
    assert (rep["attempts"], rep["skipped"], rep["consecutive"], rep["last_skipped_attempt"]) == (2, 1, 0, 0)
    assert rep["elements"] == {} and rep["since_last_report"] == {"skipped": 0, "elements": {}, "norm_overflow": False}
    # both go on alike
    for m, o in ((model, opt), (model2, opt2)):
        E._feed(m, g, has)
        o.step(grad_clip=CLIP)
    torch.cuda.synchronize()
    assert _same(opt.flat_p, opt2.flat_p) and _same(opt.exp_avg_sq, opt2.exp_avg_sq) and int(opt2.step_t) == 2
    assert opt2.state_dict()["nonfinite"] == {"skipped": 1, "attempts": 3}
    # torch.optim.AdamW takes the dict and drops the key; an optimizer without the guard ignores it, one with it
    # counts from zero when the key is missing
    shadows = [p.detach().clone().requires_grad_() for p in gb.params]
    ref = torch.optim.AdamW(shadows, lr=1e-3, weight_decay=1e-2)
    ref.load_state_dict(sd)
    assert "nonfinite" not in ref.state_dict() and len(ref.state_dict()["state"]) == len(sd["state"])
    model3, _ = E._model()
    off_opt = E._make_opt(model3, "default")
    off_opt.load_state_dict(sd)
    assert "nonfinite" not in off_opt.state_dict() and int(off_opt.step_t) == 1
    opt2.load_state_dict({k: v for k, v in sd.items() if k != "nonfinite"})
    assert opt2.skipped_updates == 0 and opt2.nonfinite_report()["attempts"] == 0


class _Recorder:
    """the library behind a proxy that notes the name of every entry point FlatAdamW asks for"""

    def __init__(self, real):
        self._real, self.names = real, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._real, name)


def test_without_the_switch_the_launch_sequence_is_the_one_without_the_feature(monkeypatch, deterministic_forward):
    from mesm_amd import optim
    from mesm_amd.graphed import StepCache
    rec = _Recorder(optim.lib())
    monkeypatch.setattr(optim, "lib", lambda: rec)

    def called():
        names, rec.names = rec.names, []
        return names

    model, crit = E._model()
    opt = E._make_opt(model, "default", ema_decay=DECAY)
    grouped_model, _ = E._model()
    grouped = E._make_opt(grouped_model, "groups")
    for o in (opt, grouped):
        assert o.skip_nonfinite is False and o.guard_tensors() == []
        assert all(getattr(o, a) is None for a in ("_guard_state", "_guard_go", "_guard_counts", "_guard_table"))
        with pytest.raises(RuntimeError, match="without skip_nonfinite"):
            o.skipped_updates
        with pytest.raises(RuntimeError, match="without skip_nonfinite"):
            o.nonfinite_report()
    E._backward(model, crit)
    called()
    opt.step()  # no clipping: no sum of squares either, the host advances the count
    assert called() == ["mesm_adamw_step_ema"] and opt.last_norm is None and int(opt.step_t) == 1
    opt.step(grad_clip=CLIP)
    assert called() == ["mesm_grad_sumsq", "mesm_adamw_step_ema"] and int(opt.step_t) == 2 and float(opt.last_norm) > 0
    E._feed(grouped_model, model.gradbuf().flat, _has_grad(model))
    grouped.step()
    grouped.step(grad_clip=CLIP)
    assert called() == ["mesm_adamw_step_groups", "mesm_grad_sumsq", "mesm_adamw_step_groups"]
    assert "nonfinite" not in opt.state_dict() and "nonfinite" not in grouped.state_dict()
    # the captured tail, each on a model of its own as in the captured tests above: two launches per pass, the gated sum
    # of squares and the gated update, and the twelve addresses it bakes in
    for form, update in (("default", "mesm_adamw_step_ema_gated"), ("groups", "mesm_adamw_step_groups_ema_gated")):
        model2, crit2 = E._model()
        opt2 = E._make_opt(model2, form, ema_decay=DECAY)
        called()
        cache = StepCache(model2, crit2, "qvhighlights", micro_steps=2, optimizer=opt2, grad_clip=CLIP)
        for b, d in E._shards():
            cache.run(b, draws=d)
        torch.cuda.synchronize()
        names = called()
        assert names and names == ["mesm_grad_sumsq_gated", update] * (len(names) // 2), names
        assert cache.update_due and int(opt2.step_t) == 1 and opt2.guard_tensors() == []
        ptrs = opt2.captured_ptrs()
        assert len(ptrs) == 12 and ptrs == [t.data_ptr() if t is not None else 0 for t in (
            opt2.flat_p, opt2.exp_avg, opt2.exp_avg_sq, opt2.step_t, opt2.lr_t, opt2._table, opt2._cap_tags,
            opt2._cap_partials, opt2._cap_norm, opt2.ema, opt2._ema_state, opt2.last_ema_decay)]
    # with the switch: the sum of squares without clipping too, the guard, the gated twin
    model3, _ = E._model()
    on = E._make_opt(model3, "default", ema_decay=DECAY, skip_nonfinite=True)
    E._feed(model3, model.gradbuf().flat, _has_grad(model))
    called()
    on.step()
    assert called() == ["mesm_grad_sumsq", "mesm_grad_guard", "mesm_adamw_step_ema_gated"]
    assert len(on.captured_ptrs()) == 16
