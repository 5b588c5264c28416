"""FlatAdamW's weight EMA (mesm_amd/optim.py: ema_decay=) on qvh_tiny weights: eager steps against the fp64 recurrence
(tests/ema_ref.py) and a twin without EMA, the captured micro-stepped update, swap_ema() for evaluation, and checkpoints.
Model in eval() mode, deterministic forward, the batches of tests/test_micro_steps_gpu.py."""
import argparse
import functools

import numpy as np
import pytest
import torch

import ema_ref
from golden_io import Fixture

pytestmark = pytest.mark.gpu

DECAY = 0.999
CLIP = 0.1


def dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


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
def _dev_batch():
    from mesm_amd import synthetic
    return synthetic.to_device(_fx().batch, dev())


def _backward(model, crit):
    """one eager forward + criterion + backward on the fixture's batch and draws: the gradients land in the flat buffer"""
    fx, batch = _fx(), _dev_batch()
    out = model(**batch, dataset_name=fx.cfg["dataset_name"], is_training=True, neg_index=fx.neg_index,
                masked_words=fx.masked_words)
    _, total = crit(out, batch, True)
    model.zero_grad(set_to_none=True)
    total.backward()


def _feed(twin, flat_grad, has_grad):
    """a recorded gradient (flat buffer, which tensors have one) as the twin model's gradient"""
    gt = twin.gradbuf()
    gt.flat.copy_(flat_grad)
    for q, on in zip(gt.params, has_grad):
        q.grad = q._mesm_gview if on else None


def _twin_step(twin, opt_t, model, clip=CLIP):
    """the gradient `model` holds, through FlatAdamW.step on the twin model"""
    gb = model.gradbuf()
    _feed(twin, gb.flat, [p.grad is not None for p in gb.params])
    opt_t.step(grad_clip=clip)


def _left_out(model):
    """a tensor every step writes a gradient for, to be left out of the grouped optimizer"""
    return next(p for n, p in model.named_parameters() if n in _fx().grads and p.ndim == 2)


def _make_opt(model, form, **ema):
    from mesm_amd.optim import FlatAdamW
    if form == "default":
        return FlatAdamW(model, lr=1e-3, weight_decay=1e-2, **ema)
    out = _left_out(model)
    rest = [p for p in model.gradbuf().params if p is not out]
    one = [p for p in rest if p.ndim > 1]
    two = [p for p in rest if p.ndim <= 1]
    return FlatAdamW(model, params=[dict(params=one, lr=1e-3, weight_decay=1e-2), dict(params=two, lr=5e-4, weight_decay=0.0)],
                     **ema)


def _decay_is(opt, want):
    """the decay the last update used is within one unit in the last place of the host mirror's"""
    got = np.float32(opt.last_ema_decay.item())
    return abs(float(got) - float(want)) <= float(np.spacing(np.float32(want)))


def _updated(model, opt):
    """per tensor of the gradient buffer: the update writes it (it has a gradient and sits in a group)"""
    return [p.grad is not None and opt._group_of[i] >= 0 for i, p in enumerate(model.gradbuf().params)]


# ------------------------------------------------------------------------------------------ 1. eager


@pytest.mark.parametrize("form", ["default", "groups"])
def test_five_eager_steps_against_the_recurrence_and_a_twin_without_ema(form, deterministic_forward):
    from mesm_amd.optim import ema_decay_at
    steps = 5
    model, crit = _model()
    twin, _ = _model()
    opt = _make_opt(model, form, ema_decay=DECAY, ema_warmup=True)
    opt_t = _make_opt(twin, form)
    assert opt.ema is not None and opt_t.ema is None and opt.ema.data_ptr() % 16 == 0
    gb = model.gradbuf()
    e0 = opt.ema.cpu().numpy()
    assert _same(opt.ema, opt.flat_p) and opt.num_updates == 0
    p_seq, decays = [], []
    for k in range(steps):
        _backward(model, crit)
        opt.step(grad_clip=CLIP)
        _twin_step(twin, opt_t, model)
        torch.cuda.synchronize()
        # the EMA entry gives the twin entry's parameters, moments, count and norm
        for a, b in ((opt.flat_p, opt_t.flat_p), (opt.exp_avg, opt_t.exp_avg), (opt.exp_avg_sq, opt_t.exp_avg_sq),
                     (opt.step_t, opt_t.step_t), (opt.last_norm, opt_t.last_norm)):
            assert _same(a, b), k
        d = np.float32(opt.last_ema_decay.item())
        assert _decay_is(opt, ema_decay_at(k, DECAY, True)), (k, float(d))
        p_seq.append(opt.flat_p.cpu().numpy())
        decays.append(d)
        assert opt.num_updates == k + 1
    assert [round(float(d), 4) for d in decays[:3]] == [0.1, 0.1818, 0.25]  # the warm-up schedule is what runs
    updated = _updated(model, opt)
    written = np.zeros(gb.numel, dtype=bool)
    for p, off, on in zip(gb.params, gb.offsets, updated):
        written[off:off + p.numel()] = on
    ref, big = ema_ref.ema_recurrence(e0, p_seq, decays, written)
    got = opt.ema.cpu().numpy()
    worst, still = (0.0, ""), []
    for name, p, off, on in zip(gb.names, gb.params, gb.offsets, updated):
        sl = slice(off, off + p.numel())
        if not on:
            continue
        err = float(np.abs(got[sl].astype(np.float64) - ref[sl]).max())
        bound = steps * ema_ref.EMA_UNITS * ema_ref.EMA_UNIT * float(big[sl].max())
        worst = max(worst, (err / (ema_ref.EMA_UNIT * max(float(big[sl].max()), 1e-30)), name))
        assert err <= bound, (name, err, bound)
        if all(np.array_equal(ps[sl], e0[sl]) for ps in p_seq):
            # a zero gradient without weight decay (unknown_token in the grouped form) never moves the parameter:
            # e == p is an exact fixed point of the update
            assert np.array_equal(got[sl].view(np.int32), e0[sl].view(np.int32)), name
            still.append(name)
        else:
            assert not np.array_equal(got[sl], p_seq[-1][sl]), name  # (an average, not a copy)
    print("%s: worst tensor %.3f units of 2^-24 * max after %d updates (bound %d): %s"
          % (form, worst[0], steps, steps * ema_ref.EMA_UNITS, worst[1]))
    # tensors the update skips -- no gradient, or (grouped) left out: the average is the parameter, the fixture's bits
    skipped = [n for n, on in zip(gb.names, updated) if not on]
    assert skipped and sum(updated) - len(still) > 10
    assert not still or form == "groups"  # (with weight decay everywhere every updated tensor moves)
    if form == "groups":
        assert any(p is _left_out(model) for p, on in zip(gb.params, updated) if not on)
    sd = opt.ema_state_dict()
    named = dict(model.named_parameters())
    for n in skipped:
        assert _same(sd[n], named[n].detach()) and torch.equal(sd[n].cpu(), _fx().sd[n]), n


# ------------------------------------------------------------------------------------------ 2. captured


@pytest.mark.parametrize("form", ["default", "groups"])
def test_captured_update_keeps_the_average_on_due_replays_only(form, deterministic_forward):
    from mesm_amd.graphed import StepCache
    model, crit = _model()
    twin, _ = _model()
    opt = _make_opt(model, form, ema_decay=DECAY)
    opt_t = _make_opt(twin, form, ema_decay=DECAY)
    cache = StepCache(model, crit, "qvhighlights", micro_steps=2, optimizer=opt, grad_clip=CLIP)
    items = _shards()
    state = lambda: [t.clone() for t in [opt.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.step_t] + opt.ema_tensors()]
    for cycle in range(2):
        before = state()
        cache.run(items[0][0], draws=items[0][1])
        torch.cuda.synchronize()
        assert not cache.update_due and opt.num_updates == cycle
        # not due: parameters, moments, count, the average and the last decay keep their bits.  The MesmEmaState words
        # (index 5) do too, except that the first replay after the host edit of cycle 0 has uploaded the new decay
        # into them -- the host's doing, not the gated launch's
        now = state()
        for i, (a, b) in enumerate(zip(now, before)):
            assert _same(a, b) or (cycle == 1 and i == 5), i
        assert _same(now[5][4:], before[5][4:])
        assert now[5][:4].view(torch.float32).item() == np.float32(DECAY if cycle == 0 else 0.9)
        cache.run(items[1][0], draws=items[1][1])
        torch.cuda.synchronize()
        assert cache.update_due and cache.updates == cycle + 1 and opt.num_updates == cycle + 1
        _twin_step(twin, opt_t, model)
        torch.cuda.synchronize()
        assert _same(opt.flat_p, opt_t.flat_p), cycle
        assert _same(opt.ema, opt_t.ema), cycle
        assert _same(opt.last_ema_decay, opt_t.last_ema_decay)
        assert not _same(opt.ema, before[4]) and not _same(opt.ema, opt.flat_p)
        assert np.float32(opt.last_ema_decay.item()) == np.float32(DECAY if cycle == 0 else 0.9), cycle  # (no arithmetic)
        if cycle == 0:
            caps = cache.captures
            opt.ema_decay = opt_t.ema_decay = 0.9  # followed at the next replay, in the same device words
    assert cache.captures == caps == 2
    # a graph captured in the middle of a cycle (its warm-up and capture passes run real updates), in a bucket never seen:
    # compared immediately around the capture, no replay and so no update due -- the average and everything else keep
    # their bits
    from mesm_amd import synthetic
    from mesm_amd.graphed import GraphedStep
    cache.run(items[0][0], draws=items[0][1])
    torch.cuda.synchronize()
    assert not cache.update_due
    before = state()
    GraphedStep(model, crit, synthetic.to_device(_batch([3, 3, 2], 41), dev()), "qvhighlights", warmup=1, micro_steps=2,
                optimizer=opt, grad_clip=CLIP)
    torch.cuda.synchronize()
    for a, b in zip(state(), before):
        assert _same(a, b)
    assert opt.num_updates == 2
    cache.reset_cycle()


# ------------------------------------------------------------------------------------------ 3. swap


def _eval_forward(model, neg):
    fx = _fx()
    with torch.no_grad():
        out = model(**_dev_batch(), dataset_name=fx.cfg["dataset_name"], is_training=False, neg_index=neg)
    return {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}


def test_swap_ema_evaluates_the_averaged_weights_in_place(deterministic_forward):
    from mesm_amd.graphed import EvalGraphedStep
    fx = _fx()
    model, crit = _model()
    opt = _make_opt(model, "default", ema_decay=0.9)
    for _ in range(2):
        _backward(model, crit)
        opt.step(grad_clip=CLIP)
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    neg = fx.neg_index
    graph = EvalGraphedStep(model, None, _dev_batch(), fx.cfg["dataset_name"], neg_index=neg.cpu().numpy())
    raw_replay = graph.replay()
    p_bits, e_bits = opt.flat_p.clone(), opt.ema.clone()
    assert not _same(p_bits, e_bits)
    ptrs = [p.data_ptr() for p in model.parameters()]
    raw = _eval_forward(model, neg)
    # a second model with the averaged weights loaded by value
    second, _ = _model()
    sd = model.state_dict()
    sd.update(opt.ema_state_dict())
    second.load_state_dict(sd)
    want = _eval_forward(second, neg)
    with opt.swap_ema():
        torch.cuda.synchronize()
        assert _same(opt.flat_p, e_bits) and _same(opt.ema, p_bits)
        assert [p.data_ptr() for p in model.parameters()] == ptrs
        got = _eval_forward(model, neg)
        assert set(got) == set(want) and "pred_spans" in got
        for k in want:
            assert _same(got[k], want[k]), k
        assert any(not _same(got[k], raw[k]) for k in raw)
        # inside the block ema_state_dict() still names the average
        inside = opt.ema_state_dict()
        assert all(_same(inside[n], sd[n]) for n in inside)
        with pytest.raises(RuntimeError, match="swap_ema"):
            opt.step(grad_clip=CLIP)
        with pytest.raises(RuntimeError, match="swap_ema"):
            with opt.swap_ema():
                pass
        swapped_replay = graph.replay()  # captured before the swap: the same addresses, now the averaged weights
    torch.cuda.synchronize()
    assert _same(opt.flat_p, p_bits) and _same(opt.ema, e_bits)
    assert [p.data_ptr() for p in model.parameters()] == ptrs
    assert torch.equal(graph.replay(), raw_replay) and not torch.equal(swapped_replay, raw_replay)
    # the same graph with the averaged weights written into the parameters by value gives the replay made inside the swap
    opt.flat_p.copy_(e_bits)
    assert torch.equal(graph.replay(), swapped_replay)
    opt.flat_p.copy_(p_bits)
    # an exception inside the block still exchanges back
    with pytest.raises(KeyError):
        with opt.swap_ema():
            raise KeyError("x")
    torch.cuda.synchronize()
    assert _same(opt.flat_p, p_bits) and _same(opt.ema, e_bits)


# ------------------------------------------------------------------------------------------ 4. checkpoints


def test_checkpoint_round_trip_weights_only_load_and_torch_interchange(tmp_path, deterministic_forward):
    from mesm_amd.checkpoint import load_checkpoint, save_checkpoint
    from mesm_amd.optim import ema_decay_at
    fx = _fx()
    model, crit = _model()
    opt = _make_opt(model, "default", ema_decay=DECAY, ema_warmup=True)
    for _ in range(2):
        _backward(model, crit)
        opt.step(grad_clip=CLIP)
    path = str(tmp_path / "ema.ckpt")
    save_checkpoint(path, model, opt, None, 0, argparse.Namespace(**fx.cfg))
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups", "ema"} and sd["ema"]["num_updates"] == 2
    assert sd["ema"]["decay"] == DECAY and sd["ema"]["warmup"] is True and len(sd["ema"]["params"]) == len(sd["state"])
    # the uninterrupted run: one more step on a recorded gradient
    _backward(model, crit)
    gb = model.gradbuf()
    g3, has3 = gb.flat.clone(), [p.grad is not None for p in gb.params]
    opt.step(grad_clip=CLIP)
    torch.cuda.synchronize()
    # the resumed run: fresh model and optimizer, the checkpoint, the same gradient
    model2, _ = _model()
    opt2 = _make_opt(model2, "default", ema_decay=0.5)  # (decay and warm-up come from the checkpoint)
    assert load_checkpoint(path, model2, opt2, None, resume_all=True) == 1
    assert opt2.num_updates == 2 and opt2.ema_decay == DECAY and opt2.ema_warmup is True
    assert not _same(opt2.ema, opt2.flat_p)  # the restored average won over the reset of the model's load
    _feed(model2, g3, has3)
    opt2.step(grad_clip=CLIP)
    torch.cuda.synchronize()
    assert _same(opt2.flat_p, opt.flat_p) and _same(opt2.ema, opt.ema)
    assert _same(opt2.last_ema_decay, opt.last_ema_decay)
    assert _decay_is(opt, ema_decay_at(2, DECAY, True)) and ema_decay_at(2, DECAY, True) == np.float32(0.25)
    assert opt2.num_updates == opt.num_updates == 3
    # weights alone, loaded after the optimizer was built: the average starts over from them
    model.load_state_dict(fx.sd)
    torch.cuda.synchronize()
    assert _same(opt.ema, opt.flat_p) and opt.num_updates == 0
    assert all(torch.equal(t.cpu(), fx.sd[n]) for n, t in opt.ema_state_dict().items())
    _feed(model, g3, has3)
    opt.step(grad_clip=CLIP)
    assert _decay_is(opt, ema_decay_at(0, DECAY, True)) and ema_decay_at(0, DECAY, True) == np.float32(0.1)
    # a state dict without the key resets, too; load_ema_state_dict is the inverse of ema_state_dict
    plain = {k: v for k, v in sd.items() if k != "ema"}
    opt.load_state_dict(plain)
    assert _same(opt.ema, opt.flat_p) and opt.num_updates == 0
    opt.load_ema_state_dict(opt2.ema_state_dict())
    assert _same(opt.ema, opt2.ema)
    # interchange: torch.optim.AdamW takes the dict (and drops the key); an optimizer without EMA ignores it
    shadows = [p.detach().clone().requires_grad_() for p in gb.params]
    ref = torch.optim.AdamW(shadows, lr=1e-3, weight_decay=1e-2)
    ref.load_state_dict(sd)
    assert "ema" not in ref.state_dict() and len(ref.state_dict()["state"]) == len(sd["state"])
    model3, _ = _model()
    off = _make_opt(model3, "default")
    off.load_state_dict(sd)
    assert off.ema is None and "ema" not in off.state_dict() and int(off.step_t) == 2
