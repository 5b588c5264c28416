"""Parameter groups and partial coverage of the flat AdamW on the device: mesm_adamw_step_groups (csrc/optim.hip) on
synthetic flat buffers against the header's formulas in float64 and against mesm_adamw_step, and FlatAdamW with groups
(mesm_amd/optim.py) against nn.utils.clip_grad_norm_ + torch.optim.AdamW with the same groups on the gradients of the
real backward (train.py:68-72)."""
import argparse
import ctypes
import functools

import pytest
import torch

from golden_io import Fixture

pytestmark = pytest.mark.gpu

BOUND = 2e-6  # max |a - b| / max |b|, the bound of tests/test_optim_gpu.py
NORM_BOUND = 1e-5


def dev():
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------ the kernel, directly

N = 1_200_128  # n / 4 = 300,032 groups of 4 > 1024 workgroups x 256 threads: the grid-stride loop wraps
SEGMENTS = (1, 1, 2, 16, 75, 257)  # run lengths in groups of 4; 352 in all, so runs start at every multiple of 32
# lr, (beta1, beta2), eps, weight_decay, step0
GROUPS = ((1e-3, (0.9, 0.999), 1e-8, 1e-2, 0),
          (1e-4, (0.8, 0.99), 1e-6, 0.0, 2),
          (0.0, (0.9, 0.999), 1e-8, 0.1, 0))


def _runs(values):
    """one tag per group of 4: consecutive runs of SEGMENTS' lengths, cycling over `values`"""
    n4 = N // 4
    reps = n4 // sum(SEGMENTS) + 1
    lens = torch.tensor(SEGMENTS * reps)
    vals = torch.tensor([values[j % len(values)] for j in range(len(lens))], dtype=torch.uint8)
    return torch.repeat_interleave(vals, lens)[:n4].contiguous()


def _table(rows):
    from mesm_amd import _lib
    arr = (_lib.AdamGroup * len(rows))()
    for r, (lr, (b1, b2), eps, wd, step0) in zip(arr, rows):
        r.lr, r.beta1, r.beta2, r.eps, r.weight_decay, r.step0 = lr, b1, b2, eps, wd, step0
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev())


def _f32(x):
    """the value the float field of the device table holds (the kernel's input), as a Python float"""
    return ctypes.c_float(x).value


@functools.lru_cache(maxsize=None)
def _inputs():
    """(p, m, v) after two imagined steps and four gradients with magnitudes log-uniform in 1e-4..1; never modified"""
    gen = torch.Generator(device=dev()).manual_seed(11)
    rnd = lambda f: f(N, device=dev(), generator=gen, dtype=torch.float32)
    p = rnd(torch.randn)
    m = 0.1 * rnd(torch.randn)
    v = 0.01 * rnd(torch.rand)
    gs = []
    for _ in range(4):
        mag = torch.pow(10.0, -4.0 * rnd(torch.rand))
        gs.append(torch.where(rnd(torch.rand) < 0.5, -mag, mag))
    return p, m, v, tuple(gs)


def _sumsq(g, step_t):
    from mesm_amd._lib import check, lib, ptr, stream_ptr
    partials = torch.empty(1024, device=dev(), dtype=torch.float32)
    n_p = ctypes.c_int32(0)
    check(lib().mesm_grad_sumsq(ptr(g), g.numel(), ptr(partials), ctypes.byref(n_p), ptr(step_t), stream_ptr()), "sumsq")
    return partials, n_p.value


def _step_groups(p, g, m, v, tags, table, n_groups, step_t, max_norm=0.0):
    """one update through the new entry; the step counter advances like FlatAdamW advances it"""
    from mesm_amd._lib import check, lib, ptr, stream_ptr
    norm = torch.zeros(1, device=dev(), dtype=torch.float32)
    if max_norm > 0:
        partials, n_p = _sumsq(g, step_t)
    else:
        partials, n_p = None, 0
        step_t += 1
    check(lib().mesm_adamw_step_groups(ptr(p), ptr(g), ptr(m), ptr(v), ptr(tags), p.numel(), ptr(partials), n_p,
                                       float(max_norm), ptr(table), n_groups, ptr(step_t), ptr(norm), stream_ptr()),
          "mesm_adamw_step_groups")
    return norm


def _step_old(p, g, m, v, active, lr_t, betas, eps, wd, step_t, max_norm=0.0):
    from mesm_amd._lib import check, lib, ptr, stream_ptr
    norm = torch.zeros(1, device=dev(), dtype=torch.float32)
    if max_norm > 0:
        partials, n_p = _sumsq(g, step_t)
    else:
        partials, n_p = None, 0
        step_t += 1
    check(lib().mesm_adamw_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(active), p.numel(), ptr(partials), n_p,
                                float(max_norm), ptr(lr_t), betas[0], betas[1], eps, wd, ptr(step_t), ptr(norm),
                                stream_ptr()), "mesm_adamw_step")
    return norm


def _ref_step(p, g, m, v, tag_el, step, coef):
    """the header's formulas in float64, in place, per element, with the float32 hyperparameters of the table"""
    for k, (lr, (b1, b2), eps, wd, step0) in enumerate(GROUPS):
        t = step - step0
        if t < 1:
            continue
        lr, b1, b2, eps, wd = (_f32(x) for x in (lr, b1, b2, eps, wd))
        sel = tag_el == k + 1
        gg = coef * g[sel]
        mk = b1 * m[sel] + (1 - b1) * gg
        vk = b2 * v[sel] + (1 - b2) * gg * gg
        pk = p[sel] * (1 - lr * wd)
        pk = pk - lr / (1 - b1 ** t) * mk / (vk.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
        p[sel], m[sel], v[sel] = pk, mk, vk


def _rel(a, b):
    return float((a.double() - b).abs().max()) / float(b.abs().max())


def _bits(x):
    return x.view(torch.int32)


def test_run_boundaries_fall_where_the_kernel_can_go_wrong():
    tags = _runs((1, 2, 3, 0)).long()
    starts = (torch.nonzero(tags[1:] != tags[:-1]).flatten() + 1)
    assert bool((starts % 64 != 0).any())  # inside a wave
    assert bool(((starts % 64 == 0) & (starts % 256 != 0)).any())  # on a wave edge
    assert bool((starts % 256 == 0).any())  # on a workgroup edge
    assert bool((starts > 1024 * 256).any())  # and in the second trip of the grid-stride loop
    assert set(tags.unique().tolist()) == {0, 1, 2, 3}


def test_three_groups_against_float64():
    """global steps 3 to 6; group 1 joined after step 2 (its t runs 1..4), group 2 has lr = 0"""
    p0, m0, v0, gs = _inputs()
    tags = _runs((1, 2, 3, 0)).to(dev())
    tag_el = tags.repeat_interleave(4)
    table = _table(GROUPS)
    step_t = torch.full((1,), 2, device=dev(), dtype=torch.int32)
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    rp, rm, rv = p0.double(), m0.double(), v0.double()
    for step, g in zip(range(3, 7), gs):
        _step_groups(p, g, m, v, tags, table, 3, step_t)
        _ref_step(rp, g.double(), rm, rv, tag_el, step, 1.0)
        assert int(step_t) == step
        errs = _rel(p, rp), _rel(m, rm), _rel(v, rv)
        print("step %d: p %.2e m %.2e v %.2e" % ((step,) + errs))
        assert max(errs) < BOUND, (step, errs)
    off, zero_lr = tag_el == 0, tag_el == 3
    assert torch.equal(_bits(p)[zero_lr], _bits(p0)[zero_lr])  # lr == 0: p bit-unchanged ...
    assert not torch.equal(m[zero_lr], m0[zero_lr]) and not torch.equal(v[zero_lr], v0[zero_lr])  # ... m, v move
    for a, b in ((p, p0), (m, m0), (v, v0)):
        assert torch.equal(_bits(a)[off], _bits(b)[off])  # tag 0: untouched
        assert not torch.equal(a[tag_el == 1], b[tag_el == 1]) and not torch.equal(a[tag_el == 2], b[tag_el == 2])


def test_young_group_is_skipped():
    """t = *step - step0 < 1 (FlatAdamW never produces it): nothing of that group moves, nothing turns non-finite"""
    p0, m0, v0, gs = _inputs()
    tags = _runs((1, 2, 3, 0)).to(dev())
    tag_el = tags.repeat_interleave(4)
    step_t = torch.full((1,), 1, device=dev(), dtype=torch.int32)  # the update below is global step 2 = group 1's step0
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    _step_groups(p, gs[0], m, v, tags, _table(GROUPS), 3, step_t)
    young = tag_el == 2
    for a, b in ((p, p0), (m, m0), (v, v0)):
        assert torch.equal(_bits(a)[young], _bits(b)[young])
        assert bool(torch.isfinite(a).all())
    assert not torch.equal(p[tag_el == 1], p0[tag_el == 1])


def test_nan_gradients_under_tag_zero_touch_nothing():
    p0, m0, v0, gs = _inputs()
    tags = _runs((1, 2, 3, 0)).to(dev())
    off = tags.repeat_interleave(4) == 0
    g = gs[0].clone()
    g[off] = float("nan")
    step_t = torch.full((1,), 2, device=dev(), dtype=torch.int32)
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    _step_groups(p, g, m, v, tags, _table(GROUPS), 3, step_t, max_norm=0.0)
    for a, b in ((p, p0), (m, m0), (v, v0)):
        assert torch.equal(_bits(a)[off], _bits(b)[off])
        assert bool(torch.isfinite(a).all())
    assert not torch.equal(m[~off], m0[~off])


def test_clip_factor_and_norm_against_float64():
    p0, m0, v0, gs = _inputs()
    tags = _runs((1, 2, 3, 0)).to(dev())
    tag_el = tags.repeat_interleave(4)
    g = gs[1]
    step_t = torch.full((1,), 2, device=dev(), dtype=torch.int32)
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    norm = _step_groups(p, g, m, v, tags, _table(GROUPS), 3, step_t, max_norm=0.1)
    assert int(step_t) == 3
    want = float(g.double().pow(2).sum().sqrt())  # the WHOLE buffer, tag 0 included
    print("norm %.9g want %.9g" % (float(norm), want))
    assert want > 1.0 and abs(float(norm) - want) < NORM_BOUND * want
    rp, rm, rv = p0.double(), m0.double(), v0.double()
    _ref_step(rp, g.double(), rm, rv, tag_el, 3, min(1.0, 0.1 / (want + 1e-6)))
    errs = _rel(p, rp), _rel(m, rm), _rel(v, rv)
    print("clipped step: p %.2e m %.2e v %.2e" % errs)
    assert max(errs) < BOUND, errs
    assert not torch.equal(m, m0)


@pytest.mark.parametrize("max_norm", [0.1, 0.0])
def test_one_group_equals_the_old_entry_bit_for_bit(max_norm):
    p0, m0, v0, gs = _inputs()
    mask = _runs((1, 1, 0, 1, 1)).to(dev())  # tag 1 = group 0 for the new entry, "active" for the old one
    lr, betas, eps, wd, _ = GROUPS[0]
    table = _table(GROUPS[:1])
    lr_t = torch.full((1,), lr, device=dev(), dtype=torch.float32)
    new = [x.clone() for x in (p0, m0, v0)]
    old = [x.clone() for x in (p0, m0, v0)]
    step_new = torch.zeros(1, device=dev(), dtype=torch.int32)
    step_old = torch.zeros(1, device=dev(), dtype=torch.int32)
    for g in gs[:3]:
        n_new = _step_groups(new[0], g, new[1], new[2], mask, table, 1, step_new, max_norm)
        n_old = _step_old(old[0], g, old[1], old[2], mask, lr_t, betas, eps, wd, step_old, max_norm)
        assert torch.equal(n_new, n_old) and (max_norm == 0 or float(n_new) > 0)
        for a, b in zip(new, old):
            assert torch.equal(_bits(a), _bits(b))
    assert int(step_new) == 3 and not torch.equal(new[0], p0)
    skipped = mask.repeat_interleave(4) == 0
    assert torch.equal(new[0][skipped], p0[skipped])


# ------------------------------------------------------------------------------------------ FlatAdamW on qvh_tiny


def _setup():
    from mesm_amd import build_criterion, build_model, synthetic
    fx = Fixture("qvh_tiny")
    args = argparse.Namespace(**fx.cfg)
    args.device = "cuda:0"
    model = build_model(args)
    model.load_state_dict(fx.sd)
    crit = build_criterion(args)
    model.eval()
    batch = synthetic.to_device(fx.batch, dev())
    return fx, model, crit, batch


def _backward(fx, model, crit, batch):
    out = model(**batch, dataset_name=fx.cfg["dataset_name"], is_training=True,
                neg_index=fx.neg_index, masked_words=fx.masked_words)
    _, total = crit(out, batch, True)
    model.zero_grad(set_to_none=True)
    total.backward()
    return float(total)


def _shadows(model):
    return {n: p.detach().clone().requires_grad_() for n, p in model.named_parameters()}


def _mirror(groups, model, shadows):
    """the same group dicts over the shadow parameters (for torch.optim.AdamW)"""
    name_of = {id(p): n for n, p in model.named_parameters()}
    return [dict(g, params=[shadows[name_of[id(p)]] for p in g["params"]]) for g in groups]


def _four_groups(model):
    """decoder at 0.1 x lr, no weight decay on the 1-d tensors of either, the SS reconstructor frozen"""
    from mesm_amd.optim import param_groups
    groups = param_groups(model, [("transformer.decoder.", dict(lr=1e-4)), ("ss_reconstructor.", dict(freeze=True))],
                          no_decay_1d=True, lr=1e-3, weight_decay=1e-2)
    assert [(g["lr"], g["weight_decay"]) for g in groups] == [(1e-3, 1e-2), (1e-3, 0.0), (1e-4, 1e-2), (1e-4, 0.0)]
    return groups


def _lambdas(n):
    return [lambda epoch, k=k: 1.0 / (1.0 + 0.5 * (k + 1) * epoch) for k in range(n)]


def _worst(model, shadows):
    worst = 0.0
    for n, p in model.named_parameters():
        a, b = p.detach().double(), shadows[n].detach().double()
        worst = max(worst, float((a - b).abs().max()) / max(float(b.abs().max()), 1e-6))
    return worst


class _Pair:
    """FlatAdamW on the model and torch.optim.AdamW on shadow parameters, fed the same gradients"""

    def __init__(self, groups_of, grad_clip=0.0, setup=None):
        from mesm_amd.optim import FlatAdamW
        self.fx, self.model, self.crit, self.batch = setup or _setup()
        self.grad_clip = grad_clip
        self.shadows = _shadows(self.model)
        groups = groups_of(self.model)
        self.opt = FlatAdamW(self.model, params=groups, lr=1e-3, weight_decay=1e-2)
        self.ref = torch.optim.AdamW(_mirror(groups, self.model, self.shadows), lr=1e-3, weight_decay=1e-2)

    def grads(self):
        _backward(self.fx, self.model, self.crit, self.batch)
        for n, p in self.model.named_parameters():
            self.shadows[n].grad = None if p.grad is None else p.grad.detach().clone()

    def ref_step(self):
        self.want_norm = None
        if self.grad_clip > 0:  # train.py:70: over every parameter that has a gradient, in the optimizer or not
            self.want_norm = torch.nn.utils.clip_grad_norm_([s for s in self.shadows.values() if s.grad is not None],
                                                            self.grad_clip)
        self.ref.step()

    def check(self, what):
        if self.grad_clip > 0:
            got, want = float(self.opt.last_norm), float(self.want_norm)
            assert abs(got - want) < NORM_BOUND * max(1.0, want), (what, got, want)
        worst = _worst(self.model, self.shadows)
        print("%s: worst %.2e" % (what, worst))
        assert worst < BOUND, (what, worst)

    def step(self, what):
        self.grads()
        self.ref_step()
        self.opt.step(grad_clip=self.grad_clip)
        self.check(what)


@pytest.mark.parametrize("form", ["FlatAdamW", "build_optimizer"])
def test_default_form_is_the_old_entry_bit_for_bit(form):
    from mesm_amd._lib import check, lib, ptr, stream_ptr
    from mesm_amd.optim import FlatAdamW, build_optimizer
    fx, model, crit, batch = _setup()
    if form == "FlatAdamW":
        opt = FlatAdamW(model, lr=1e-3, weight_decay=1e-2)
    else:
        opt, _ = build_optimizer(argparse.Namespace(lr=1e-3, weight_decay=1e-2, lr_drop=100, gamma=0.1), model)
    gb = model.gradbuf()
    start = model.flat_params().clone()
    p, m, v = start.clone(), torch.zeros_like(start), torch.zeros_like(start)
    step_t = torch.zeros(1, device=dev(), dtype=torch.int32)
    lr_t = torch.full((1,), 1e-3, device=dev(), dtype=torch.float32)
    for grad_clip in (0.1, 0.0, 0.1):
        _backward(fx, model, crit, batch)
        active = torch.zeros(gb.numel // 4, dtype=torch.uint8)
        for q, off in zip(gb.params, gb.offsets):
            if q.grad is not None:
                active[off // 4:(off + q.numel() + 3) // 4] = 1
        assert 0 < int(active.sum()) < active.numel()
        _step_old(p, gb.flat, m, v, active.to(dev()), lr_t, (0.9, 0.999), 1e-8, 1e-2, step_t, grad_clip)
        opt.step(grad_clip=grad_clip)
        assert torch.equal(_bits(model.flat_params()), _bits(p))
        assert torch.equal(_bits(opt.exp_avg), _bits(m)) and torch.equal(_bits(opt.exp_avg_sq), _bits(v))
    assert not torch.equal(p, start)


@pytest.mark.parametrize("grad_clip", [0.1, 0.0])
def test_four_groups_match_torch(grad_clip):
    pair = _Pair(_four_groups, grad_clip)
    sched = torch.optim.lr_scheduler.LambdaLR(pair.opt, _lambdas(4))
    ref_sched = torch.optim.lr_scheduler.LambdaLR(pair.ref, _lambdas(4))
    for step in range(4):
        pair.step("step %d" % step)
        sched.step(); ref_sched.step()
        assert [g["lr"] for g in pair.opt.param_groups] == [g["lr"] for g in pair.ref.param_groups]
    lrs = [g["lr"] for g in pair.opt.param_groups]
    assert len(set(lrs)) == 4 and lrs[0] < 1e-3  # every group went its own way
    moved = frozen = gradless = 0
    for n, p in pair.model.named_parameters():
        same = torch.equal(p.detach().cpu(), pair.fx.sd[n].cpu())
        if n.startswith("ss_reconstructor."):
            assert same, n  # frozen: untouched, gradient or not
            frozen += p.grad is not None
        elif p.grad is None:
            assert same, n  # no gradient: no decay either, like torch skips p.grad is None
            gradless += 1
        else:
            moved += not same
    assert frozen > 0 and gradless > 0 and moved > 50


def test_edits_between_steps_reach_the_device():
    pair = _Pair(_four_groups, 0.1)
    for step in range(4):
        if step == 2:
            for opt in (pair.opt, pair.ref):
                opt.param_groups[0]["weight_decay"] = 0.3
                opt.param_groups[0]["betas"] = (0.7, 0.95)
                opt.param_groups[0]["eps"] = 1e-3
        pair.step("step %d" % step)  # (weight_decay 0.3 at lr 1e-3 alone moves a parameter by 3e-4 of itself per step)


def test_add_param_group_after_two_steps():
    from mesm_amd.optim import param_groups

    def without_head(model):
        return param_groups(model, [("output_txt_proj.", dict(freeze=True))], lr=1e-3, weight_decay=1e-2)

    pair = _Pair(without_head, 0.1)
    head = [(n, p) for n, p in pair.model.named_parameters() if n.startswith("output_txt_proj.")]
    assert len(head) == 6 and len(pair.opt.param_groups) == 1
    for step in range(2):
        pair.step("step %d" % step)
    for n, p in head:
        assert torch.equal(p.detach().cpu(), pair.fx.sd[n].cpu()) and p.grad is not None, n
    pair.opt.add_param_group({"params": [p for _, p in head], "lr": 5e-4})
    pair.ref.add_param_group({"params": [pair.shadows[n] for n, _ in head], "lr": 5e-4})
    assert pair.opt.param_groups[1]["weight_decay"] == 1e-2  # from the defaults
    for step in range(2, 4):
        pair.step("step %d" % step)
    for n, p in head:
        assert not torch.equal(p.detach().cpu(), pair.fx.sd[n].cpu()), n
    sd = pair.opt.state_dict()
    assert [len(g["params"]) for g in sd["param_groups"]] == [len(pair.model.gradbuf().params) - 6, 6]
    for k, want in ((0, 4.0), (1, 2.0)):
        for pid in sd["param_groups"][k]["params"]:
            assert float(sd["state"][pid]["step"]) == want, (k, pid)
    ref_sd = pair.ref.state_dict()
    assert float(ref_sd["state"][sd["param_groups"][1]["params"][0]]["step"]) == 2.0


def test_checkpoint_interchange_with_torch():
    from mesm_amd.optim import FlatAdamW
    pair = _Pair(_four_groups, 0.1)
    for step in range(3):
        pair.step("step %d" % step)
    flat_sd, torch_sd = pair.opt.state_dict(), pair.ref.state_dict()
    assert [g["params"] for g in flat_sd["param_groups"]] == [g["params"] for g in torch_sd["param_groups"]]
    assert float(flat_sd["state"][0]["step"]) == 3.0
    groups = _four_groups(pair.model)
    # FlatAdamW's state into a fresh torch optimizer over second shadows ...
    shadows2 = _shadows(pair.model)
    ref2 = torch.optim.AdamW(_mirror(groups, pair.model, shadows2), lr=1.0, weight_decay=0.5)
    ref2.load_state_dict(flat_sd)
    # ... and torch's state into a fresh FlatAdamW, which takes the model over
    opt2 = FlatAdamW(pair.model, params=groups, lr=1.0, weight_decay=0.5)
    opt2.load_state_dict(torch_sd)
    assert [g["lr"] for g in opt2.param_groups] == [g["lr"] for g in pair.ref.param_groups] == [1e-3, 1e-3, 1e-4, 1e-4]
    assert [g["weight_decay"] for g in ref2.param_groups] == [1e-2, 0.0, 1e-2, 0.0]
    pair.opt = opt2
    for step in range(3, 5):
        pair.grads()
        for n, s in pair.shadows.items():
            shadows2[n].grad = None if s.grad is None else s.grad.clone()
        pair.ref_step()
        torch.nn.utils.clip_grad_norm_([s for s in shadows2.values() if s.grad is not None], 0.1)
        ref2.step()
        opt2.step(grad_clip=0.1)
        pair.check("step %d, torch -> flat" % step)
        worst = _worst(pair.model, shadows2)
        print("step %d, flat -> torch: worst %.2e" % (step, worst))
        assert worst < BOUND, (step, worst)
    assert float(opt2.state_dict()["state"][0]["step"]) == 5.0


def test_captured_step_follows_the_host_hyperparameters():
    """opt.step(grad_clip) captured once (two launches in a row) and replayed on fresh gradients; the twin is
    torch.optim.AdamW stepping eagerly on shadow parameters, as in the tests above.  The learning rates change before
    every replay and reach the replayed kernel through the device table alone."""
    pair = _Pair(_four_groups, 0.1)
    sched = torch.optim.lr_scheduler.LambdaLR(pair.opt, _lambdas(4))
    ref_sched = torch.optim.lr_scheduler.LambdaLR(pair.ref, _lambdas(4))
    pair.step("eager warm-up")  # the tag and hyperparameter tensors exist from here on
    tags, table = pair.opt._tags().data_ptr(), pair.opt._table.data_ptr()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=side):
        pair.opt.step(grad_clip=0.1)
    assert int(pair.opt.step_t) == 1  # capturing ran nothing
    for replay in range(3):
        sched.step(); ref_sched.step()
        pair.opt.sync_hyperparameters()
        pair.grads()
        pair.ref_step()
        graph.replay()
        pair.check("replay %d" % replay)
    assert int(pair.opt.step_t) == 4
    assert (pair.opt._tags().data_ptr(), pair.opt._table.data_ptr()) == (tags, table)
    assert pair.opt.param_groups[0]["lr"] < 0.5e-3
