"""Micro-batched graph replays (mesm_amd/graphed.py: GraphedStep / StepCache with micro_steps=k): k replays accumulate the
MEAN of their gradients in the flat buffer, and with optimizer= the clip + AdamW update is captured behind the backward and
acts on the last replay of a cycle only.  qvh_tiny weights, the five-group synthetic batch of
test_graph_ddp_gpu.py::test_two_shards_mean_equals_oracle_mean, model in eval() mode, deterministic forward."""
import argparse
import functools

import pytest
import torch

from golden_io import Fixture

pytestmark = pytest.mark.gpu

GRAD_BOUND = 5e-4    # per tensor against the oracle: the bound of the eager two-shard test for the same quantities
REPLAY_BOUND = 1e-4  # |got - ref| / |ref| on the flat buffer: tests/test_autograph_gpu.py, replayed against eager
PARAM_BOUND = 2e-6   # per tensor, max |a - b| / max |b|: tests/test_optim_gpu.py::test_flat_adamw_matches_torch


def dev():
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-3)


def flat_rel(got, ref):
    return float((got.double() - ref.double()).norm()) / max(float(ref.double().norm()), 1e-12)


@functools.lru_cache(maxsize=None)
def _fx():
    return Fixture("qvh_tiny")


def _model():
    from mesm_amd import build_criterion, build_model
    fx = _fx()
    a = argparse.Namespace(**fx.cfg)
    a.device = "cuda:0"
    model = build_model(a)
    model.load_state_dict(fx.sd)
    crit = build_criterion(a)
    model.eval()
    return model, crit


def _batch(groups, seed):
    from mesm_amd import synthetic
    c = _fx().cfg
    return synthetic.make_batch("qvhighlights", groups, c["Lv"], c["Lw"], c["v_feat_dim"], c["t_feat_dim"],
                                c["vocab_size"] + 1, seed=seed, ragged=True)


@functools.lru_cache(maxsize=None)
def _shards():
    """the two shards (5 and 2 pairs) of the five-group batch with their host draws; never modified"""
    from mesm_amd import synthetic
    from mesm_amd.ddp import shard_groups
    batch = _batch([2, 1, 2, 1, 1], 21)
    shards = [shard_groups(batch, r, 2) for r in range(2)]
    return tuple((s, synthetic.host_draws(s, seed=r)) for r, s in enumerate(shards))


@functools.lru_cache(maxsize=None)
def _oracle_mean():
    """mean over the shards of the oracle's per-shard gradients: {name: tensor} over the tensors either shard reaches"""
    from oracle import mesm_oracle as O
    fx = _fx()
    grads = [O.train_step(fx.sd, fx.cfg, s, neg, masked)[3] for s, (neg, masked) in _shards()]
    names = set(grads[0]) | set(grads[1])
    zero = lambda n: torch.zeros_like(fx.sd[n])
    return {n: (grads[0].get(n, zero(n)).double() + grads[1].get(n, zero(n)).double()) / 2 for n in names}


def _cycle(cache, items):
    """one replay per (batch, draws); -> the GraphedSteps that served them"""
    return [cache.run(b, draws=d)[1] for b, d in items]


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def test_two_shards_through_the_graphs_equal_the_oracle_mean(deterministic_forward):
    from mesm_amd.graphed import StepCache
    model, crit = _model()
    cache = StepCache(model, crit, "qvhighlights", micro_steps=2)
    assert cache.micro_steps == 2 and not cache.update_due
    ora = _oracle_mean()
    for cycle in range(2):  # (the first one captures both graphs, the second of them in the middle of the cycle)
        g0, g1 = _cycle(cache, _shards())
        assert g0 is not g1 and g0._cycle is g1._cycle and cache.captures == 2
        assert cache.update_due and g1.update_due
        torch.cuda.synchronize()
        got = _grads(model)
        assert set(got) == set(ora), sorted(set(got) ^ set(ora))
        worst = max((rel(got[n], ora[n]), n) for n in ora)
        print("cycle %d: worst tensor %.2e (%s)" % (cycle, worst[0], worst[1]))
        assert worst[0] < GRAD_BOUND, worst
    # half a cycle, dropped: the next replay clears the buffer
    cache.run(_shards()[0][0], draws=_shards()[0][1])
    assert not cache.update_due
    cache.reset_cycle()
    _cycle(cache, _shards())
    assert cache.update_due
    got = _grads(model)
    worst = max((rel(got[n], ora[n]), n) for n in ora)
    assert worst[0] < GRAD_BOUND, worst
    assert cache._cycle.words.tolist()[:2] == [0, 2]
    assert cache.updates == 0  # no optimizer captured: the caller steps


@functools.lru_cache(maxsize=None)
def _three():
    from mesm_amd import synthetic
    bs = [_batch([2, 1, 2], 31 + i) for i in range(3)]
    return tuple((b, synthetic.host_draws(b, seed=10 + i)) for i, b in enumerate(bs))


def test_three_micro_steps_equal_the_mean_of_single_step_graphs(deterministic_forward):
    from mesm_amd.graphed import StepCache
    model, crit = _model()
    flat = model.gradbuf
    plain = StepCache(model, crit, "qvhighlights")  # the single-step graphs as they were: one gradient at a time
    ref = None
    for b, d in _three():
        _, gs = plain.run(b, draws=d)
        assert gs._cycle is None
        torch.cuda.synchronize()
        g = flat().flat.double()
        ref = g if ref is None else ref + g
    ref = ref / 3
    cache = StepCache(model, crit, "qvhighlights", micro_steps=3)
    for cycle in range(2):
        steps = _cycle(cache, _three())
        assert cache.update_due and cache.captures == len({id(s) for s in steps})
        torch.cuda.synchronize()
        err = flat_rel(flat().flat, ref)
        print("cycle %d: |got - ref| / |ref| = %.2e" % (cycle, err))
        assert err < REPLAY_BOUND, err
    # k changes at a boundary without a new capture: two of the three batches, mean over two
    ref2 = None
    for b, d in _three()[:2]:
        plain.run(b, draws=d)
        torch.cuda.synchronize()
        g = flat().flat.double()
        ref2 = g if ref2 is None else ref2 + g
    caps = cache.captures
    cache.set_micro_steps(2)
    _cycle(cache, _three()[:2])
    assert cache.update_due and cache.captures == caps
    torch.cuda.synchronize()
    err = flat_rel(flat().flat, ref2 / 2)
    print("k = 2 after k = 3: %.2e" % err)
    assert err < REPLAY_BOUND, err


def _twin_step(twin, opt_t, model, clip=0.1):
    """the gradient `model`'s cycle left, through the existing FlatAdamW.step on the twin model"""
    gb, gt = model.gradbuf(), twin.gradbuf()
    gt.flat.copy_(gb.flat)
    for p, q in zip(gb.params, gt.params):
        q.grad = q._mesm_gview if p.grad is not None else None
    opt_t.step(grad_clip=clip)


def _worst_param(model, twin):
    worst = (0.0, "")
    for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        a, b = p.detach().double(), q.detach().double()
        worst = max(worst, (float((a - b).abs().max()) / max(float(b.abs().max()), 1e-6), n))
    return worst


def _state(opt):
    return [t.clone() for t in (opt.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.step_t)]


def _left_out(model):
    """a tensor every step writes a gradient for, to be left out of the grouped optimizer"""
    return next(p for n, p in model.named_parameters() if n in _fx().grads and p.ndim == 2)


def _make_opt(model, form):
    from mesm_amd.optim import FlatAdamW
    if form == "default":
        return FlatAdamW(model, lr=1e-3, weight_decay=1e-2)
    out = _left_out(model)
    rest = [p for p in model.gradbuf().params if p is not out]
    one = [p for p in rest if p.ndim > 1]
    two = [p for p in rest if p.ndim <= 1]
    return FlatAdamW(model, params=[dict(params=one, lr=1e-3, weight_decay=1e-2), dict(params=two, lr=5e-4, weight_decay=0.0)])


@pytest.mark.parametrize("form", ["default", "groups"])
def test_captured_update_acts_on_the_last_replay_of_a_cycle_only(form, deterministic_forward):
    from mesm_amd.graphed import StepCache
    fx = _fx()
    model, crit = _model()
    twin, _ = _model()
    opt, opt_t = _make_opt(model, form), _make_opt(twin, form)
    sched = torch.optim.lr_scheduler.StepLR(opt, 1, gamma=0.5)
    sched_t = torch.optim.lr_scheduler.StepLR(opt_t, 1, gamma=0.5)
    cache = StepCache(model, crit, "qvhighlights", micro_steps=2, optimizer=opt, grad_clip=0.1)
    items = _shards()
    moved = []
    for cycle in range(2):
        before = _state(opt)
        cache.run(items[0][0], draws=items[0][1])
        torch.cuda.synchronize()
        assert not cache.update_due and cache.updates == cycle
        for a, b in zip(_state(opt), before):  # not due: parameters, both moments and the step count keep their bits
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        cache.run(items[1][0], draws=items[1][1])
        torch.cuda.synchronize()
        assert cache.update_due and cache.updates == cycle + 1 and int(opt.step_t) == cycle + 1
        _twin_step(twin, opt_t, model)
        torch.cuda.synchronize()
        worst = _worst_param(model, twin)
        print("%s, cycle %d: worst parameter %.2e (%s), norm %.6f" % (form, cycle, worst[0], worst[1], float(opt.last_norm)))
        assert worst[0] < PARAM_BOUND, worst
        assert abs(float(opt.last_norm) - float(opt_t.last_norm)) <= 1e-6 * float(opt_t.last_norm)
        moved.append(float((opt.flat_p - before[0]).abs().max()))
        if cycle == 0:
            caps = cache.captures
            sched.step(); sched_t.step()  # the rate halves: the next update follows it without a new capture
    assert cache.captures == caps == 2
    assert opt.param_groups[0]["lr"] == 0.5e-3
    assert 0 < moved[1] < 0.75 * moved[0], moved  # AdamW moves an element by about lr per step
    # tensors no graph writes a gradient for (and, grouped, the one left out) keep the fixture's bits: no decay either
    untouched = [n for n, p in model.named_parameters() if p.grad is None]
    if form == "groups":
        untouched += [n for n, p in model.named_parameters() if p is _left_out(model)]
    assert untouched
    for n, p in model.named_parameters():
        if n in untouched:
            assert torch.equal(p.detach().cpu(), fx.sd[n]), n
    # the default form's by-value hyperparameters cannot change under a captured update
    if form == "default":
        opt.param_groups[0]["weight_decay"] = 0.5
        with pytest.raises(RuntimeError, match="fixed in a captured update"):
            cache.run(items[0][0], draws=items[0][1])
        opt.param_groups[0]["weight_decay"] = 1e-2


def test_a_graph_captured_in_the_middle_of_a_cycle_leaves_the_cycle_alone(deterministic_forward):
    """Micro-step 2 of 2 arrives in a bucket never seen, against the same cycle with both graphs warm.

    The two runs compute their gradients separately, so these agree to the order of the backward's atomic float sums, not
    bit for bit, and the parameters are compared after an AdamW step on them.  AdamW divides every element by its own
    magnitude: an element whose gradient is analytically zero (the attention key biases: softmax does not see them) carries
    rounding noise only, and with eps below that noise it moves by up to lr in a noise-determined direction
    (tests/test_graph_ddp_gpu.py::test_graph_with_flat_adamw_trains_like_eager bounds those tensors apart for that reason).
    For the per-tensor bound of 2e-6 to say something about the CAPTURE, eps has to sit above the noise of the clipped
    gradient: float32 rounding (6e-8) of gradient elements up to ~1, times the clip factor 0.1 / |g| with |g| in the tens,
    is ~1e-10; an element then differs by at most lr * 1e-10 / eps between the runs, and lr = 1e-3, eps = 1e-5 keeps that
    at 1e-8, under 2e-6 of a tensor whose largest entry is 1e-2.  A stray update from the capture's warm-up passes would
    still move elements by 2e-5 .. 1e-3 (clipped gradient elements of 2e-7 .. 2e-4 against that eps), two orders above
    the bound.  (With the default eps = 1e-8 the same comparison measures 4.6e-5 on
    transformer.encoder.layers.1.self_attn.in_proj_bias, gradients 2.0e-8 apart.)"""
    from mesm_amd.graphed import StepCache
    from mesm_amd.optim import FlatAdamW
    fx = _fx()
    items = _shards()
    res = []
    for warm in (False, True):
        model, crit = _model()
        opt = FlatAdamW(model, lr=1e-3, weight_decay=1e-2, eps=1e-5)
        cache = StepCache(model, crit, "qvhighlights", micro_steps=2, optimizer=opt, grad_clip=0.1)
        if warm:  # both graphs exist before the cycle that counts; then weights and optimizer state start over
            _cycle(cache, items)
            torch.cuda.synchronize()
            model.load_state_dict(fx.sd)
            opt.exp_avg.zero_(); opt.exp_avg_sq.zero_(); opt.step_t.zero_()
            assert cache.captures == 2
        _cycle(cache, items)
        torch.cuda.synchronize()
        assert cache.captures == 2 and cache.update_due and int(opt.step_t) == 1
        res.append((model.gradbuf().flat.clone(), {n: p.detach().clone() for n, p in model.named_parameters()}))
    (g_cold, p_cold), (g_warm, p_warm) = res
    err = flat_rel(g_cold, g_warm)
    print("gradients, captured mid-cycle against warm: %.2e" % err)
    assert err < REPLAY_BOUND, err
    worst = max((float((p_cold[n].double() - p_warm[n].double()).abs().max())
                 / max(float(p_warm[n].double().abs().max()), 1e-6), n) for n in p_warm)
    print("parameters: worst %.2e (%s)" % worst)
    assert worst[0] < PARAM_BOUND, worst


def test_controls(deterministic_forward):
    from mesm_amd import synthetic
    from mesm_amd.graphed import GraphedStep, SplitGraphedStep, StepCache
    from mesm_amd.optim import FlatAdamW
    model, crit = _model()
    (b0, d0), (b1, d1) = _shards()
    # the default: the graph as it was, no cycle state anywhere
    plain = GraphedStep(model, crit, synthetic.to_device(b0, dev()), "qvhighlights", warmup=1)
    plain.set_draws(*d0)
    plain.run(redraw=False)
    torch.cuda.synchronize()
    ref = model.gradbuf().flat.clone()
    assert plain._cycle is None and model.gradbuf().cycle is None and plain.micro_steps is None and not plain.update_due
    with pytest.raises(RuntimeError):
        plain.set_micro_steps(2)
    # k = 1 without an optimizer is that graph plus the gate
    one = GraphedStep(model, crit, synthetic.to_device(b0, dev()), "qvhighlights", warmup=1, micro_steps=1)
    one.set_draws(*d0)
    for _ in range(2):
        one.run(redraw=False)
        assert one.update_due
    torch.cuda.synchronize()
    assert flat_rel(model.gradbuf().flat, ref) < REPLAY_BOUND
    assert model.gradbuf().cycle is one._cycle
    # set_micro_steps in the middle of a cycle
    one.set_micro_steps(3)
    one.run(redraw=False)
    with pytest.raises(RuntimeError, match="cycle boundary"):
        one.set_micro_steps(2)
    one.reset_cycle()
    one.set_micro_steps(1)
    one.run(redraw=False)
    torch.cuda.synchronize()
    assert one.update_due and flat_rel(model.gradbuf().flat, ref) < REPLAY_BOUND
    # refusals, each with its reason
    class Reducer:
        expected = None

        def backward_scale(self):
            return 1.0

    with pytest.raises(ValueError, match="reducer"):
        StepCache(model, crit, "qvhighlights", reducer=Reducer(), micro_steps=2)
    with pytest.raises(ValueError, match="reducer"):
        GraphedStep(model, crit, synthetic.to_device(b0, dev()), "qvhighlights", reducer=Reducer(), micro_steps=2)
    with pytest.raises(ValueError, match="one-graph step"):
        SplitGraphedStep(model, crit, synthetic.to_device(b0, dev()), "qvhighlights", micro_steps=2)
    other, _ = _model()
    with pytest.raises(ValueError, match="does not cover this model's flat buffers"):
        StepCache(model, crit, "qvhighlights", micro_steps=2, optimizer=FlatAdamW(other, lr=1e-3))
    with pytest.raises(ValueError, match="needs micro_steps"):
        StepCache(model, crit, "qvhighlights", optimizer=FlatAdamW(model, lr=1e-3))
    with pytest.raises(ValueError, match=">= 1"):
        StepCache(model, crit, "qvhighlights", micro_steps=0)
