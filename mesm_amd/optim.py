"""Optimizer tail of the reference train loop on the flat buffers.

    train.py:68-72     optimizer.zero_grad(); loss.backward();
                       nn.utils.clip_grad_norm_(model.parameters(), opt.grad_clip); optimizer.step()
    runner.py:348-352  AdamW(lr, weight_decay) + StepLR(lr_drop, gamma)

The model's gradients already live in ONE flat fp32 buffer (gradbuf.py).  FlatAdamW moves the
parameters into a second flat buffer with the same layout (every `param.data` becomes a view, so the
modules, state_dict() and checkpoints are unaffected), keeps exp_avg / exp_avg_sq flat as well, and
runs clipping + the AdamW update for all 273 tensors in two kernel launches (csrc/optim.hip)
instead of ~8 foreach launches over 262 views.  Step count and learning rate are device scalars,
so `step()` can be captured in the same HIP graph as the training step.

Drop-in use in the reference loop:

    optimizer, lr_scheduler = build_optimizer(opt, model)        # this module's build_optimizer
    ...
    optimizer.zero_grad(); loss.backward()
    optimizer.step(grad_clip=opt.grad_clip)     # replaces clip_grad_norm_ + optimizer.step()

`clip_grad_norm_(model, max_norm)` is also provided for loops that keep the two calls apart.

Parameter groups (the `param_dicts` form of runner.py:349) and partial coverage:

    groups = param_groups(model, [("transformer.decoder.", dict(lr=0.1 * opt.lr)),
                                  ("ss_reconstructor.", dict(freeze=True))],
                          no_decay_1d=True, lr=opt.lr, weight_decay=opt.weight_decay)
    optimizer = FlatAdamW(model, params=groups)                  # or params=[some parameters]

Still two launches: one tag byte per 4 elements of the flat layout names the group (0: not covered, or no
gradient this step), and lr / betas / eps / weight_decay of every group live in a small device table, so
a captured `step()` follows what schedulers and users write into `param_groups`.

Weight EMA (`ema_decay=`): an exponential moving average of the parameters, kept by the SAME update launch in a third
flat buffer -- train on the raw weights, evaluate and checkpoint the averaged ones:

    optimizer = FlatAdamW(model, lr=opt.lr, ema_decay=0.999, ema_warmup=True)
    ...
    with optimizer.swap_ema():              # the parameters hold the average inside the block; no address moves
        eval_epoch(model, ...)

Non-finite gradients (`skip_nonfinite=True`): one more launch between the sum of squares and the update (mesm_grad_guard)
looks at the total norm ON THE DEVICE; when it is inf or NaN the update is skipped as a whole -- parameters, moments, EMA and
step count keep their bits -- and the tensors that hold the bad elements are counted, with no host synchronisation:

    optimizer = FlatAdamW(model, lr=opt.lr, skip_nonfinite=True)
    ...
    if it % 1000 == 0 and optimizer.skipped_updates:        # (reads one device word)
        print(optimizer.nonfinite_report()["since_last_report"])

Per-tensor statistics (`tensor_stats=k`): at every k-th update attempt one more launch in front of the update
(mesm_tensor_stats) reduces the gradient and the parameter buffer per tensor -- sum of squares in fp64, largest magnitude --
into device memory; nothing is read back until the caller asks:

    optimizer = FlatAdamW(model, lr=opt.lr, tensor_stats=100)
    ...
    rep = optimizer.tensor_stats()          # synchronises; {"samples", "attempt", "total_grad_norm", "tensors", "groups"}
"""
import contextlib
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr


def _sumsq(gb, step_t=None):
    flat = gb.flat
    partials = torch.empty(1024, device=flat.device, dtype=torch.float32)
    np_out = ctypes.c_int32(0)
    check(lib().mesm_grad_sumsq(ptr(flat), flat.numel(), ptr(partials), ctypes.byref(np_out), ptr(step_t),
                                stream_ptr()), "mesm_grad_sumsq")
    return partials, np_out.value


def clip_grad_norm_(model, max_norm):
    """nn.utils.clip_grad_norm_(model.parameters(), max_norm) on the flat gradient buffer (two
    launches).  Returns the total norm as a device scalar (no host sync)."""
    gb = model.gradbuf()
    partials, n_p = _sumsq(gb)
    norm = torch.empty(1, device=gb.flat.device, dtype=torch.float32)
    check(lib().mesm_clip_grad(ptr(gb.flat), gb.flat.numel(), ptr(partials), n_p, float(max_norm), ptr(norm),
                               stream_ptr()), "mesm_clip_grad")
    return norm[0]


_HYPER = ("lr", "betas", "eps", "weight_decay")
_TABLE_SLOTS = 4  # pinned staging copies of the hyperparameter table in flight at once


def tag_table(gb, group_of, has_grad):
    """The uint8 table mesm_adamw_step_groups reads, on the host: one byte per 4 elements of the flat layout
    (gradbuf.py pads every tensor to a multiple of 4, so no byte belongs to two tensors), group index + 1 over the
    padded range of every tensor that sits in a group AND has a gradient, 0 everywhere else."""
    tags = torch.zeros(gb.numel // 4, dtype=torch.uint8)
    for p, off, k, on in zip(gb.params, gb.offsets, group_of, has_grad):
        if on and k >= 0:
            tags[off // 4:(off + p.numel() + 3) // 4] = k + 1
    return tags


def segment_table(gb):
    """The tensors of a GradBuffer as mesm_grad_guard's segment table, on the host: (starts, order).  `starts` (int32,
    len(gb.params) + 1 entries) holds the first float4 of every tensor in ascending order plus the end of the buffer --
    gradbuf.py pads every tensor to a multiple of 4 elements and leaves no gap, so segment j is float4s
    [starts[j], starts[j + 1]) -- and `order[j]` is the index of segment j's tensor in gb.names / gb.params.  Packs permute
    the offsets, so the table is NOT in parameter order."""
    order = sorted(range(len(gb.params)), key=lambda i: gb.offsets[i])
    starts = [gb.offsets[i] // 4 for i in order] + [gb.numel // 4]
    for j, i in enumerate(order):
        assert gb.offsets[i] % 4 == 0 and gb.offsets[i] + (gb.params[i].numel() + 3) // 4 * 4 == 4 * starts[j + 1], gb.names[i]
    return torch.tensor(starts, dtype=torch.int32), order


def check_guard_segments(n_seg, what="skip_nonfinite: the non-finite guard (mesm_grad_guard) names the tensors at fault"):
    """the limit of mesm_grad_guard and mesm_tensor_stats on the number of segments, in words"""
    if not 1 <= n_seg <= _lib.GUARD_MAX_SEGMENTS:
        raise _lib.MesmError("%s through a table of 1 to %d segments, and the gradient buffer holds %d tensors"
                             % (what, _lib.GUARD_MAX_SEGMENTS, n_seg))


def _check_stats_every(every, least):
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or not least <= every < 2 ** 31:
        raise ValueError("tensor_stats takes None or an int >= 1 (sample every that many update attempts; the attribute "
                         "tensor_stats_every also takes 0, which pauses sampling), got %r" % (every,))
    return int(every)


def reduce_stat_slots(starts, n4, n_wg, sumsq, absmax):
    """mesm_tensor_stats' result tables -> per segment, on the host.  `starts`: the n_seg + 1 float4 starts of the segment
    table; `n4`: float4s in the flat buffers; `n_wg`: the workgroups of the launch (mesm_tensor_stats_workgroups), each of
    which reduced C = ceil(n4 / n_wg) consecutive float4s and left its part of segment s in slot s + b; `sumsq` (float64)
    and `absmax` (uint32): the 2 * (n_seg + n_wg) entries each, g first, then p.  Returns (sumsq, absmax) of shape
    (2, n_seg): the parts of every segment added (maximum taken) in ascending workgroup order, so the same raw tables
    always give the same bits; an empty segment gives 0."""
    starts = np.asarray(starts, dtype=np.int64)
    n_seg = len(starts) - 1
    n_slots = n_seg + n_wg
    sumsq = np.asarray(sumsq, dtype=np.float64).reshape(2, n_slots)
    absmax = np.asarray(absmax, dtype=np.uint32).reshape(2, n_slots)
    chunk = -(-int(n4) // int(n_wg))
    full = starts[1:] > starts[:-1]
    first = np.where(full, starts[:-1] // chunk, 0)
    count = np.where(full, (starts[1:] - 1) // chunk - first + 1, 0)
    seg = np.repeat(np.arange(n_seg), count)
    ramp = np.arange(len(seg)) - np.repeat(np.cumsum(count) - count, count)
    slot = seg + np.repeat(first, count) + ramp
    out_s = np.zeros((2, n_seg), dtype=np.float64)
    out_m = np.zeros((2, n_seg), dtype=np.uint32)
    for x in range(2):
        np.add.at(out_s[x], seg, sumsq[x, slot])  # (unbuffered, in the order of `seg`: ascending workgroups)
        np.maximum.at(out_m[x], seg, absmax[x, slot])
    return out_s, out_m


def tensor_stats_report(names, order, group_of, n_groups, has_grad, samples, attempt, sumsq, absmax):
    """FlatAdamW.tensor_stats()'s dict from per-segment arrays (reduce_stat_slots), on the host.  `names`, `group_of` (-1: in
    no group) and `has_grad` are in parameter order (gb.names); `order[j]` is the parameter of segment j (segment_table:
    packs permute the offsets); `sumsq` / `absmax` have shape (2, n_seg), gradient first.  Norms are square roots of fp64
    sums; a group's are those of its tensors' sums, and "total_grad_norm" that of all segments -- the whole buffer, like
    `last_norm`.  absmax comes back as the float whose bits it is (a NaN for a NaN).  Before the first sample the report is
    empty."""
    if samples <= 0:
        return {"samples": 0, "attempt": int(attempt), "total_grad_norm": None, "tensors": {}, "groups": []}
    sumsq = np.asarray(sumsq, dtype=np.float64)
    mag = np.ascontiguousarray(np.asarray(absmax, dtype=np.uint32)).view(np.float32)
    tensors = {}
    group_sums = np.zeros((n_groups, 2), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j, i in enumerate(order):
            tensors[names[i]] = {"grad_norm": float(np.sqrt(sumsq[0, j])), "grad_absmax": float(mag[0, j]),
                                 "param_norm": float(np.sqrt(sumsq[1, j])), "param_absmax": float(mag[1, j]),
                                 "has_grad": bool(has_grad[i]) if has_grad is not None else None}
            if group_of[i] >= 0:
                group_sums[group_of[i]] += sumsq[:, j]
        total = float(np.sqrt(np.sum(sumsq[0])))
        groups = [{"grad_norm": float(np.sqrt(g)), "param_norm": float(np.sqrt(p))} for g, p in group_sums]
    return {"samples": int(samples), "attempt": int(attempt), "total_grad_norm": total, "tensors": tensors, "groups": groups}


def _v_scale(beta2, t):
    """exp_avg_sq of torch.optim.AdamW over exp_avg_sq of the kernels after t steps on the same gradients.  The kernels
    take beta2 as a float and weigh g^2 with 1.0f - beta2 (for 0.999: 1.3e-5 below torch's 0.001) next to a bias
    correction from the same float, so their v / (1 - beta2^t) is torch's although their raw v is not; a state dict
    carries the raw moment across, and this factor keeps the bias-corrected one -- what the update uses -- intact."""
    if t < 1:
        return 1.0
    b2f = ctypes.c_float(beta2).value
    return (1.0 - beta2 ** t) / (1.0 - b2f ** t)


def ema_decay_at(n, decay, warmup):
    """The decay of the EMA update that follows `n` earlier ones, as numpy.float32: the host mirror of the kernels'
    expression (csrc/optim.hip: ema_decay), operation for operation.  Without warm-up it is `decay`; with it the average
    starts close to the weights and settles: min(decay, (1 + n) / (10 + n))."""
    d = np.float32(decay)
    if not warmup:
        return d
    nf = np.float32(max(int(n), 0))
    return np.minimum(d, (np.float32(1.0) + nf) / (np.float32(10.0) + nf))


def _check_ema_decay(decay):
    d = ctypes.c_float(float(decay)).value  # (what the kernel sees)
    if not 0.0 < d < 1.0:
        raise ValueError("ema_decay must satisfy 0 < ema_decay < 1 as a float32, got %r" % (decay,))
    return float(decay)


class FlatAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW semantics (decoupled weight decay, bias correction, eps outside the sqrt of
    the bias-corrected second moment, amsgrad off) over flat buffers.

    `params=None` covers every tensor of `model.gradbuf()` with one set of hyperparameters (one launch of
    mesm_adamw_step).  `params` may also be an iterable of parameters (a subset: the rest of the model is never
    touched) or a list of torch-style group dicts with their own lr / betas / eps / weight_decay (at most 64;
    `param_groups()` below builds such a list from name rules); the update is then mesm_adamw_step_groups, which
    reads every group's hyperparameters from a small device table.  Groups are honoured or refused (ValueError),
    never ignored: a tensor the flat buffers do not hold, a tensor in two groups, amsgrad, maximize.

    The table is uploaded by `sync_hyperparameters()` only when `param_groups` changed on the host (a scheduler,
    or the user editing weight_decay / betas / eps), into the SAME device tensor: `step()` calls it; a caller that
    replays a captured `step()` calls it before the replay.  Hyperparameter changes never need a new capture.  A
    MEMBERSHIP change does (`add_param_group`, or another set of tensors without a gradient): the tag table is
    rebuilt on the host.

    `state_dict()` / `load_state_dict()` speak torch.optim.AdamW's format with the same grouping, in both directions;
    with groups, exp_avg_sq is written in torch's convention (`_v_scale`).

    `ema_decay=d` (None: off, and nothing below exists) keeps e = d * e + (1 - d) * p in a flat buffer `ema` for every
    element an update writes, inside the update's own launch (the *_ema entries); tensors an update skips keep their
    average.  With `ema_warmup` the n-th update uses min(d, (1 + n) / (10 + n)) (`ema_decay_at`).  `ema_decay` and
    `ema_warmup` are attributes: an edit reaches the device with the next `sync_hyperparameters()`, in the same device
    words, so a captured update follows it without a new capture; `last_ema_decay` is the decay the last update used (a
    device scalar).  The average starts as a copy of the weights and starts over (`reset_ema()`) whenever
    `model.load_state_dict` brings other weights.  `swap_ema()` exchanges weights and average in place for evaluation,
    `ema_state_dict()` gives the average under the model's key names, and `state_dict()` carries it under "ema".

    `skip_nonfinite=True` (False: nothing below exists, and every launch sequence is the one without it) skips an update
    whose total gradient norm is inf or NaN, on the device.  step() and step_gated() then always run the sum of squares,
    mesm_grad_guard behind it, and the `_gated` twin of the update entry behind a device word `go` that the guard writes: a
    skipped update leaves parameters, moments, EMA, `last_ema_decay` and the step count (so bias corrections, every group's
    step0 and `num_updates`) as if the batch had never been seen; `last_norm` shows the non-finite norm.  The norm is that
    of the WHOLE flat gradient buffer, as for clipping: a non-finite element in a tensor this optimizer does not cover
    skips the update as well.  `skipped_updates` reads one device word; `nonfinite_report()` names the tensors whose
    gradients held inf / NaN and how many elements each, or says that the sum of squares overflowed over finite elements.
    `state_dict()` carries {"skipped", "attempts"} under "nonfinite".  As with torch's GradScaler, a host LR scheduler knows
    nothing of a skip and keeps stepping.

    `tensor_stats=k` (None: nothing below exists, and every launch sequence is the one without it; otherwise an int >= 1)
    puts one launch, mesm_tensor_stats, behind the sum of squares and the guard and in front of the update.  At every k-th
    update ATTEMPT -- the guard's attempt count with skip_nonfinite, so a skipped attempt is sampled like any other and its
    inf / NaN are reported as they are; the step count without -- it reduces the flat gradient buffer as the update is
    about to see it (unclipped; the mean of a micro-step cycle) and the parameters as they are before the update, per
    tensor, to a sum of squares in fp64 and a largest magnitude; at the other attempts, and in a captured tail at the
    replays that are not due, it writes nothing.  `tensor_stats()` reads the last sample back (it synchronises).
    `tensor_stats_every` is an attribute: an edit reaches the device with the next `sync_hyperparameters()`, in the same
    device word, so a captured tail follows it without a new capture; 0 pauses sampling.  The whole buffer is reduced, as
    for `last_norm`: a tensor without a gradient reports what the buffer holds, and "has_grad" is what the host knew at
    the last eager step (`p.grad is not None`) or `set_coverage()`.  `state_dict()` does not carry the statistics."""

    def __init__(self, model, params=None, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 amsgrad=False, maximize=False, ema_decay=None, ema_warmup=False, skip_nonfinite=False,
                 tensor_stats=None):
        self.skip_nonfinite = bool(skip_nonfinite)
        self._stats_on = tensor_stats is not None
        self._stats_every = _check_stats_every(tensor_stats, 1) if self._stats_on else None
        self._stats_state = self._stats_sumsq = self._stats_absmax = self._stats_table = None
        self._stats_order = self._stats_starts = self._stats_host = self._stats_has_grad = None
        self._stats_wg = 0
        self._guard_state = self._guard_go = self._guard_counts = self._guard_table = None
        self._guard_order = self._guard_last = None
        self._ema_on = ema_decay is not None
        self._ema_decay = _check_ema_decay(ema_decay) if self._ema_on else None
        self.ema_warmup = bool(ema_warmup)
        self.ema = self._ema_state = self.last_ema_decay = None
        self._ema_step0 = 0
        self._ema_host = None
        self._swapped = False
        self.model = model
        gb = model.gradbuf()
        self.gb = gb
        self._index = {id(p): i for i, p in enumerate(gb.params)}
        self._group_of = [-1] * len(gb.params)  # parameter (gradbuf order) -> its group, -1: not covered
        self._step0 = []  # per group: the global step count when it joined
        self._grouped = params is not None
        self.flat_p = self.exp_avg = self.exp_avg_sq = None
        self.step_t = self.lr_t = None
        self._active = None
        self._active_key = None
        self._table = self._table_host = self._table_events = None
        self._table_slot = 0
        self._hyper_host = None
        self.last_norm = None
        self._cap_tags = self._cap_partials = self._cap_norm = self._cap_baked = None
        if params is None:
            groups = [{"params": list(gb.params)}]
        else:
            groups = list(params)
            if groups and not isinstance(groups[0], dict):
                groups = [{"params": groups}]
        super().__init__(groups, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                                      maximize=maximize))
        if gb.params[0].is_cuda:
            # the flat state is created NOW, not at the first step(): a HIP graph captured after this
            # constructor sees the final parameter addresses (model.flat_params is idempotent and
            # build_model has normally done it already)
            self._ensure()
        if self._ema_on:
            # other weights loaded into the model later must not leave a stale average behind (a resumed optimizer state
            # is loaded after the model and puts its own average back: checkpoint.load_checkpoint)
            model.register_load_state_dict_post_hook(lambda module, incompatible: self.reset_ema())

    # ------------------------------------------------------------------ groups
    def _name_of(self, p):
        i = self._index.get(id(p))
        if i is not None:
            return self.gb.names[i]
        for n, q in self.model.named_parameters():
            if q is p:
                return n
        return "<a %s tensor that is no parameter of the model>" % (tuple(p.shape),)

    def add_param_group(self, param_group):
        """torch's add_param_group with the checks of the constructor.  A group added after construction starts its
        bias correction at t = 1 (step0 = the current step count) on zeroed moments, like torch's per-parameter
        `step`.  A captured step() must be captured again afterwards (the set of updated tensors changed)."""
        if not isinstance(param_group, dict):
            raise TypeError("param_group must be a dict")
        ps = param_group["params"]
        param_group = dict(param_group, params=[ps] if isinstance(ps, torch.Tensor) else list(ps))
        k = len(self._step0)
        if k >= _lib.ADAM_MAX_GROUPS:
            raise ValueError("FlatAdamW takes at most %d parameter groups (group %d starts with %s)"
                             % (_lib.ADAM_MAX_GROUPS, k, self._name_of(param_group["params"][0])
                                if param_group["params"] else "no parameter"))
        seen = set()
        for p in param_group["params"]:
            i = self._index.get(id(p))
            if i is None:
                raise ValueError("parameter %s is not in the model's flat buffers (not a parameter of this model, or "
                                 "requires_grad was False when the model was built)" % self._name_of(p))
            if self._group_of[i] >= 0 or i in seen:
                raise ValueError("parameter %s appears in more than one parameter group" % self.gb.names[i])
            seen.add(i)
        merged = dict(self.defaults, **param_group)
        for flag in ("amsgrad", "maximize"):
            if merged.get(flag):
                raise ValueError("FlatAdamW has no %s (group %d, which starts with %s)"
                                 % (flag, k, self._name_of(merged["params"][0]) if merged["params"] else "no parameter"))
        super().add_param_group(param_group)
        step0 = int(self.step_t.item()) if self.step_t is not None else 0
        self._step0.append(step0)
        for i in seen:
            self._group_of[i] = k
            if self.exp_avg is not None:
                sl = slice(self.gb.offsets[i], self.gb.offsets[i] + self.gb.params[i].numel())
                self.exp_avg[sl].zero_()
                self.exp_avg_sq[sl].zero_()
        self._active_key = None
        self._hyper_host = None

    # ------------------------------------------------------------------ flat state
    def _ensure(self):
        gb = self.gb
        dev = next(iter(gb.params)).device
        gb.ensure(dev)
        flat = self.model.flat_params()  # every param.data is a view of it (no-op when already flat)
        if self.flat_p is flat:
            return
        self.flat_p = flat
        self.exp_avg = torch.zeros_like(self.flat_p)
        self.exp_avg_sq = torch.zeros_like(self.flat_p)
        self.step_t = torch.zeros(1, device=dev, dtype=torch.int32)
        self.lr_t = torch.full((1,), float(self.param_groups[0]["lr"]), device=dev, dtype=torch.float32)
        if self._ema_on:
            self.ema = self.flat_p.clone()
            self._ema_state = torch.zeros(ctypes.sizeof(_lib.EmaState), device=dev, dtype=torch.uint8)
            self.last_ema_decay = torch.zeros(1, device=dev, dtype=torch.float32)
            self._ema_step0, self._ema_host = 0, None
            self._sync_ema()  # (the device words are valid from here on, whoever reads or snapshots them)
        if self.skip_nonfinite:
            table, self._guard_order = segment_table(gb)
            check_guard_segments(len(self._guard_order))
            self._guard_table = table.to(dev)
            self._guard_state = torch.zeros(4, device=dev, dtype=torch.int32)  # MesmGuardState
            self._guard_go = torch.zeros(1, device=dev, dtype=torch.int32)
            self._guard_counts = torch.zeros(len(self._guard_order), device=dev, dtype=torch.int64)
            self._guard_last = None
        if self._stats_on:
            table, self._stats_order = segment_table(gb)
            n_seg = len(self._stats_order)
            check_guard_segments(n_seg, "tensor_stats: mesm_tensor_stats reduces the tensors")
            self._stats_starts = table.numpy().astype(np.int64)
            self._stats_table = self._guard_table if self._guard_table is not None else table.to(dev)
            self._stats_wg = int(lib().mesm_tensor_stats_workgroups(gb.numel))
            if self._stats_wg < 1:
                raise _lib.MesmError("mesm_tensor_stats_workgroups failed with status %d" % self._stats_wg)
            n_slots = n_seg + self._stats_wg
            self._stats_state = torch.zeros(4, device=dev, dtype=torch.int32)  # MesmStatsState
            self._stats_sumsq = torch.zeros(2 * n_slots, device=dev, dtype=torch.float64)
            self._stats_absmax = torch.zeros(2 * n_slots, device=dev, dtype=torch.int32)  # (bits: read as uint32)
            self._stats_host = None
            self._sync_stats()
        if self._grouped:
            nbytes = _lib.ADAM_MAX_GROUPS * ctypes.sizeof(_lib.AdamGroup)
            self._table = torch.zeros(nbytes, device=dev, dtype=torch.uint8)
            self._table_host = torch.zeros(_TABLE_SLOTS, nbytes, dtype=torch.uint8)
            if dev.type == "cuda":
                self._table_host = self._table_host.pin_memory()
            self._table_events = [None] * _TABLE_SLOTS
            self._hyper_host = None
            self._active = self._active_key = None

    def _active_mask(self):
        """groups of 4 elements that belong to a parameter whose .grad is not None this step"""
        gb = self.gb
        key = tuple(p.grad is not None for p in gb.params)
        if key != self._active_key:
            mask = torch.zeros(gb.numel // 4, dtype=torch.uint8)
            for p, off, on in zip(gb.params, gb.offsets, key):
                if on:
                    mask[off // 4:(off + p.numel() + 3) // 4] = 1
            self._active = mask.to(self.flat_p.device)
            self._active_key = key
        return self._active

    def _tags(self):
        """tag_table() on the device, rebuilt when the set of tensors with a gradient (or a group's membership)
        changed; always the same device tensor"""
        key = tuple(p.grad is not None for p in self.gb.params)
        if key != self._active_key:
            tags = tag_table(self.gb, self._group_of, key)
            if self._active is None:
                self._active = tags.to(self.flat_p.device)
            else:
                self._active.copy_(tags)
            self._active_key = key
        return self._active

    def _hyper(self):
        res = []
        for g, step0 in zip(self.param_groups, self._step0):
            if g.get("amsgrad") or g.get("maximize"):
                raise ValueError("FlatAdamW has no amsgrad / maximize (group that starts with %s)"
                                 % self._name_of(g["params"][0]))
            b1, b2 = g["betas"]
            res.append((float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"]), step0))
        return res

    def sync_hyperparameters(self):
        """Bring the device-side hyperparameters up to date with `param_groups` (schedulers and users edit those on
        the host).  Costs a comparison of a few floats per group when nothing changed; otherwise one small copy from
        a pinned buffer into the same device tensor, so a captured step() sees the new values at its next replay."""
        self._ensure()
        if self._ema_on:
            self._sync_ema()
        if self._stats_on:
            self._sync_stats()
        if not self._grouped:
            g = self.param_groups[0]
            if float(g["lr"]) != getattr(self, "_lr_host", None):  # StepLR edits param_groups[0]["lr"]
                self._lr_host = float(g["lr"])
                self.lr_t.fill_(self._lr_host)
            return
        hyper = self._hyper()
        if hyper == self._hyper_host:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the hyperparameters changed: call sync_hyperparameters() before capturing step()")
        slot = self._table_slot
        self._table_slot = (slot + 1) % _TABLE_SLOTS
        if self._table_events[slot] is None:
            self._table_events[slot] = torch.cuda.Event()
        else:
            self._table_events[slot].synchronize()  # (the copy that last read this slot: long done)
        host = self._table_host[slot]
        rows = (_lib.AdamGroup * _lib.ADAM_MAX_GROUPS).from_address(host.data_ptr())
        for row, (lr, b1, b2, eps, wd, step0) in zip(rows, hyper):
            row.lr, row.beta1, row.beta2, row.eps, row.weight_decay, row.step0 = lr, b1, b2, eps, wd, step0
        self._table.copy_(host, non_blocking=True)
        self._table_events[slot].record()
        self._hyper_host = hyper

    # ------------------------------------------------------------------ weight EMA
    @property
    def ema_decay(self):
        return self._ema_decay

    @ema_decay.setter
    def ema_decay(self, value):
        if not self._ema_on:
            raise RuntimeError("FlatAdamW was built without ema_decay: there is no EMA buffer to average into")
        self._ema_decay = _check_ema_decay(value)

    def _sync_ema(self):
        """decay, warm-up switch and starting step into the device's MesmEmaState when they changed on the host"""
        cur = (self._ema_decay, bool(self.ema_warmup), self._ema_step0)
        if cur == self._ema_host:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the EMA settings changed: call sync_hyperparameters() before capturing step()")
        st = _lib.EmaState(decay=cur[0], warmup=int(cur[1]), step0=cur[2], reserved=0)
        self._ema_state.copy_(torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8))
        self._ema_host = cur

    def _ema_args(self):
        if self._swapped:
            raise RuntimeError("FlatAdamW: no update inside swap_ema() (the parameters hold the average)")
        return ptr(self.ema), ptr(self._ema_state), ptr(self.last_ema_decay)

    def _need_ema(self, what):
        if not self._ema_on:
            raise RuntimeError("FlatAdamW.%s: the optimizer was built without ema_decay" % what)
        self._ensure()

    def ema_tensors(self):
        """what the EMA adds to the optimizer's device state ([] when it is off): the average, the MesmEmaState words and
        the decay of the last update"""
        return [self.ema, self._ema_state, self.last_ema_decay] if self.ema is not None else []

    @property
    def num_updates(self):
        """EMA updates since the average was last set equal to the weights (reads the device's step count)"""
        self._need_ema("num_updates")
        return int(self.step_t.item()) - self._ema_step0

    @torch.no_grad()
    def reset_ema(self):
        """ema := the current weights, and the warm-up schedule starts over"""
        if not self._ema_on:
            raise RuntimeError("FlatAdamW.reset_ema: the optimizer was built without ema_decay")
        if self.flat_p is None:  # (no flat state yet: the average will start as a copy of whatever the weights are then)
            return
        if self._swapped:
            raise RuntimeError("FlatAdamW.reset_ema: not inside swap_ema()")
        self.ema.copy_(self.flat_p)
        self._ema_step0 = int(self.step_t.item())
        self._sync_ema()

    def _swap(self):
        check(lib().mesm_swap_f32(ptr(self.flat_p), ptr(self.ema), self.flat_p.numel(), stream_ptr()), "mesm_swap_f32")

    @contextlib.contextmanager
    def swap_ema(self):
        """Inside the block the parameters hold the averaged weights and `ema` holds the raw ones: the CONTENTS of the two
        flat buffers are exchanged (one launch) and exchanged back on exit.  No address moves, so modules, views and
        every captured training or evaluation graph stay valid.  step(), step_gated() and replays of a captured update
        raise RuntimeError inside; so does nesting."""
        self._need_ema("swap_ema")
        if self._swapped:
            raise RuntimeError("FlatAdamW.swap_ema: already inside swap_ema()")
        self._swap()
        self._swapped = True
        try:
            yield self
        finally:
            self._swap()
            self._swapped = False

    def _ema_src(self):
        return self.flat_p if self._swapped else self.ema

    def ema_state_dict(self):
        """{name: averaged tensor} for every tensor of the gradient buffer, named and shaped as in model.state_dict():
        `sd = model.state_dict(); sd.update(optimizer.ema_state_dict())` loads into this model or the reference's"""
        self._need_ema("ema_state_dict")
        gb, src = self.gb, self._ema_src()
        return {n: src[off:off + p.numel()].view(p.shape).clone() for n, p, off in zip(gb.names, gb.params, gb.offsets)}

    @torch.no_grad()
    def load_ema_state_dict(self, sd):
        """the inverse of ema_state_dict(): every tensor of the gradient buffer must be there; other keys (buffers,
        frozen tensors) are ignored"""
        self._need_ema("load_ema_state_dict")
        gb, dst = self.gb, self._ema_src()
        missing = [n for n in gb.names if n not in sd]
        if missing:
            raise KeyError("load_ema_state_dict: %d tensors missing, the first is %s" % (len(missing), missing[0]))
        for n, p, off in zip(gb.names, gb.params, gb.offsets):
            if tuple(sd[n].shape) != tuple(p.shape):
                raise ValueError("load_ema_state_dict: %s has shape %s, the model's is %s"
                                 % (n, tuple(sd[n].shape), tuple(p.shape)))
            dst[off:off + p.numel()].copy_(sd[n].reshape(-1))

    # ------------------------------------------------------------------ non-finite guard
    def guard_tensors(self):
        """what skip_nonfinite adds to the optimizer's device state ([] when it is off): the MesmGuardState words, the `go`
        word the guarded update is gated by and the per-tensor element counts (the segment table is constant)"""
        if self._guard_state is None:
            return []
        return [self._guard_state, self._guard_go, self._guard_counts]

    def _need_guard(self, what):
        if not self.skip_nonfinite:
            raise RuntimeError("FlatAdamW.%s: the optimizer was built without skip_nonfinite" % what)
        self._ensure()

    def _guard(self, partials, n_p, due, norm):
        """mesm_grad_guard behind a sum of squares -> the device word that gates the update"""
        flat = self.gb.flat
        check(lib().mesm_grad_guard(ptr(flat), flat.numel(), ptr(self._guard_table), len(self._guard_order), ptr(partials),
                                    n_p, ptr(due), ptr(self.step_t), ptr(self._guard_state), ptr(self._guard_go), ptr(norm),
                                    ptr(self._guard_counts), stream_ptr()), "mesm_grad_guard")
        return self._guard_go

    @property
    def skipped_updates(self):
        """updates skipped over a non-finite gradient norm so far (reads one device word: synchronises)"""
        self._need_guard("skipped_updates")
        return int(self._guard_state[1].item())

    def nonfinite_report(self):
        """The guard's counters (synchronises): attempts (updates applied + skipped), skipped, consecutive (skipped since the
        last applied one), last_skipped_attempt (1-based, 0: none), and under "elements" {tensor name: non-finite gradient
        elements seen in skipped updates}, cumulative, tensors without any left out.  "since_last_report" holds the
        difference to the previous call (the host keeps the last copy): "skipped", "elements", and "norm_overflow" -- True
        when updates were skipped and no count moved, i.e. the sum of squares overflowed over finite elements."""
        self._need_guard("nonfinite_report")
        st = [int(x) for x in self._guard_state.tolist()]
        counts = np.array(self._guard_counts.tolist(), dtype=np.int64)
        last_skipped, last_counts = self._guard_last or (0, np.zeros_like(counts))
        self._guard_last = (st[1], counts)
        names = [self.gb.names[i] for i in self._guard_order]
        delta = counts - last_counts
        return {"attempts": st[0], "skipped": st[1], "consecutive": st[2], "last_skipped_attempt": st[3],
                "elements": {n: int(c) for n, c in zip(names, counts) if c},
                "since_last_report": {"skipped": st[1] - last_skipped,
                                      "elements": {n: int(d) for n, d in zip(names, delta) if d},
                                      "norm_overflow": bool(st[1] > last_skipped and not delta.any())}}

    # ------------------------------------------------------------------ per-tensor statistics
    @property
    def tensor_stats_every(self):
        """sample at every that many update attempts (0: paused); None without the switch"""
        return self._stats_every

    @tensor_stats_every.setter
    def tensor_stats_every(self, value):
        if not self._stats_on:
            raise RuntimeError("FlatAdamW was built without tensor_stats: there is nothing to sample into")
        self._stats_every = _check_stats_every(value, 0)

    def _sync_stats(self):
        """the sampling interval into the first word of the device's MesmStatsState when it changed on the host (the other
        words are the device's own)"""
        if self._stats_every == self._stats_host:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("tensor_stats_every changed: call sync_hyperparameters() before capturing step()")
        self._stats_state[:1].fill_(self._stats_every)
        self._stats_host = self._stats_every

    def tensor_stat_tensors(self):
        """what tensor_stats adds to the optimizer's device state ([] when it is off): the MesmStatsState words and the two
        result tables (the segment table is constant)"""
        if self._stats_state is None:
            return []
        return [self._stats_state, self._stats_sumsq, self._stats_absmax]

    def _stats(self, due, has_grad):
        """mesm_tensor_stats behind the sum of squares and the guard, in front of the update"""
        flat = self.gb.flat
        index = self._guard_state if self.skip_nonfinite else self.step_t  # (MesmGuardState starts with `attempts`)
        self._stats_has_grad = has_grad
        check(lib().mesm_tensor_stats(ptr(flat), ptr(self.flat_p), flat.numel(), ptr(self._stats_table),
                                      len(self._stats_order), ptr(due), ptr(index), ptr(self._stats_state),
                                      ptr(self._stats_sumsq), ptr(self._stats_absmax), stream_ptr()), "mesm_tensor_stats")

    def tensor_stats(self):
        """The last sample (synchronises): {"samples": samples taken so far, "attempt": the attempt the last one saw (the
        guard's count with skip_nonfinite, the step count without), "total_grad_norm": of the whole gradient buffer,
        "tensors": {name: {"grad_norm", "grad_absmax", "param_norm", "param_absmax", "has_grad"}} for every tensor of the
        gradient buffer, "groups": [{"grad_norm", "param_norm"}] per parameter group}.  See tensor_stats_report."""
        if not self._stats_on:
            raise RuntimeError("FlatAdamW.tensor_stats: the optimizer was built without tensor_stats")
        self._ensure()
        st = [int(x) for x in self._stats_state.tolist()]
        if st[1] <= 0:
            return tensor_stats_report(self.gb.names, self._stats_order, self._group_of, len(self._step0), None, 0, st[2],
                                       None, None)
        sumsq, absmax = reduce_stat_slots(self._stats_starts, self.gb.numel // 4, self._stats_wg,
                                          self._stats_sumsq.cpu().numpy(), self._stats_absmax.cpu().numpy().view(np.uint32))
        return tensor_stats_report(self.gb.names, self._stats_order, self._group_of, len(self._step0), self._stats_has_grad,
                                   st[1], st[2], sumsq, absmax)

    def _update_guarded(self, tags, partials, n_p, clip, norm, go, ema, baked=None):
        """the `_gated` twin of the update entry that the form (default / groups) and `ema` select, gated by the guard's word"""
        name = "mesm_adamw_step"
        if self._grouped:
            name += "_groups"
            hyper = (ptr(self._table), len(self._step0))
        else:
            if baked is None:
                g = self.param_groups[0]
                baked = (float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]))
            hyper = (ptr(self.lr_t), *baked)
        name += "_ema_gated" if ema is not None else "_gated"
        args = (ptr(self.flat_p), ptr(self.gb.flat), ptr(self.exp_avg), ptr(self.exp_avg_sq), ptr(tags), self.flat_p.numel(),
                ptr(partials), n_p, clip, *hyper, ptr(self.step_t), ptr(norm), ptr(go), *(ema or ()))
        check(getattr(lib(), name)(*args, stream_ptr()), name)

    def _step_guarded(self, grad_clip):
        """step() with skip_nonfinite: sum of squares (always), guard, gated update on the guard's word"""
        ema = self._ema_args() if self._ema_on else None  # (refuses inside swap_ema() before anything is written)
        self.sync_hyperparameters()
        active = self._tags() if self._grouped else self._active_mask()
        clip = float(grad_clip or 0.0)
        partials, n_p = _sumsq(self.gb, self.step_t)
        self.last_norm = torch.empty(1, device=self.flat_p.device, dtype=torch.float32)
        go = self._guard(partials, n_p, None, self.last_norm)
        if self._stats_on:
            self._stats(None, self._active_key)
        self._update_guarded(active, partials, n_p, clip if clip > 0 else 0.0, self.last_norm, go, ema)

    def _step_gated_guarded(self, due, grad_clip):
        """step_gated() with skip_nonfinite: gated sum of squares, guard on the same `due`, gated update on the guard's word"""
        ema = self._ema_args() if self._ema_on else None
        if not torch.cuda.is_current_stream_capturing():
            self.sync_hyperparameters()
        n_p = ctypes.c_int32(0)
        flat = self.gb.flat
        check(lib().mesm_grad_sumsq_gated(ptr(flat), flat.numel(), ptr(self._cap_partials), ctypes.byref(n_p),
                                          ptr(self.step_t), ptr(due), stream_ptr()), "mesm_grad_sumsq_gated")
        clip = float(grad_clip or 0.0)
        self.last_norm = self._cap_norm
        go = self._guard(self._cap_partials, n_p.value, due, self._cap_norm)
        if self._stats_on:
            self._stats(due, self._stats_has_grad)
        if not self._grouped:
            g = self.param_groups[0]
            self._cap_baked = (float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]))
        self._update_guarded(self._cap_tags, self._cap_partials, n_p.value, clip if clip > 0 else 0.0, self._cap_norm, go, ema,
                             self._cap_baked)

    # ------------------------------------------------------------------ optimizer protocol
    @torch.no_grad()
    def step(self, closure=None, grad_clip=0.0):
        """grad_clip > 0 fuses nn.utils.clip_grad_norm_(model.parameters(), grad_clip) into the update (the
        gradients themselves are left unscaled).  The norm is that of the WHOLE flat gradient buffer, whichever
        tensors this optimizer covers.  With skip_nonfinite the sum of squares runs without clipping too, the guard behind
        it, and the update is the gated entry behind the guard's word (_step_guarded)."""
        assert closure is None
        if self.skip_nonfinite:
            return self._step_guarded(grad_clip)
        ema = self._ema_args() if self._ema_on else None  # (refuses inside swap_ema() before anything is written)
        self.sync_hyperparameters()
        active = self._tags() if self._grouped else self._active_mask()
        if grad_clip and grad_clip > 0:
            partials, n_p = _sumsq(self.gb, self.step_t)
            self.last_norm = torch.empty(1, device=self.flat_p.device, dtype=torch.float32)
        else:
            partials, n_p = None, 0
            self.step_t += 1
            self.last_norm = None
        if self._stats_on:
            self._stats(None, self._active_key)
        if self._grouped:
            args = (ptr(self.flat_p), ptr(self.gb.flat), ptr(self.exp_avg), ptr(self.exp_avg_sq), ptr(active),
                    self.flat_p.numel(), ptr(partials), n_p, float(grad_clip or 0.0), ptr(self._table), len(self._step0),
                    ptr(self.step_t), ptr(self.last_norm))
            if ema is not None:
                check(lib().mesm_adamw_step_groups_ema(*args, *ema, stream_ptr()), "mesm_adamw_step_groups_ema")
            else:
                check(lib().mesm_adamw_step_groups(*args, stream_ptr()), "mesm_adamw_step_groups")
            return
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        args = (ptr(self.flat_p), ptr(self.gb.flat), ptr(self.exp_avg), ptr(self.exp_avg_sq), ptr(active),
                self.flat_p.numel(), ptr(partials), n_p, float(grad_clip or 0.0), ptr(self.lr_t), float(b1), float(b2),
                float(g["eps"]), float(g["weight_decay"]), ptr(self.step_t), ptr(self.last_norm))
        if ema is not None:
            check(lib().mesm_adamw_step_ema(*args, *ema, stream_ptr()), "mesm_adamw_step_ema")
        else:
            check(lib().mesm_adamw_step(*args, stream_ptr()), "mesm_adamw_step")

    # ------------------------------------------------------------------ the tail captured in a micro-stepped graph
    def set_coverage(self, has_grad):
        """Which tensors a CAPTURED update covers (graphed.GraphedStep(optimizer=...)): has_grad[i] for parameter i of
        the gradient buffer -- some graph of the model writes its gradient -- instead of `p.grad is not None` at the time
        of the call, which a replay cannot look at.  The mask / tag table of the captured launches is ONE device tensor,
        rewritten in place (never from inside a capture), as are the partial sums and the norm (`last_norm`)."""
        self._ensure()
        gb = self.gb
        host = tag_table(gb, self._group_of if self._grouped else [0] * len(gb.params), tuple(has_grad))
        if self._stats_on:
            self._stats_has_grad = tuple(bool(x) for x in has_grad)
        dev = self.flat_p.device
        if self._cap_tags is None:
            self._cap_tags = host.to(dev)
            self._cap_partials = torch.zeros(1024, device=dev, dtype=torch.float32)
            self._cap_norm = torch.zeros(1, device=dev, dtype=torch.float32)
        else:
            self._cap_tags.copy_(host)

    def captured_ptrs(self):
        """addresses a captured tail bakes in (GraphedStep compares them before every replay)"""
        ts = (self.flat_p, self.exp_avg, self.exp_avg_sq, self.step_t, self.lr_t, self._table, self._cap_tags,
              self._cap_partials, self._cap_norm, self.ema, self._ema_state, self.last_ema_decay)
        if self.skip_nonfinite:
            ts += (*self.guard_tensors(), self._guard_table)
        if self._stats_on:
            ts += (*self.tensor_stat_tensors(), self._stats_table)
        return [t.data_ptr() if t is not None else 0 for t in ts]

    @torch.no_grad()
    def step_gated(self, due, grad_clip=0.0):
        """`step(grad_clip=...)` as launches that act only when the device word `due` (int32, CycleState.due_word) is set:
        otherwise nothing is written -- parameters, moments, step count and norm stay as they are.  Two launches, fixed
        tensors only, so the pair can sit in a graph that is replayed at every micro-step.  The sum of squares runs
        without clipping too: it is what advances the step count under the gate.  Coverage comes from set_coverage().
        The default form reads lr from the device; betas, eps and weight_decay are launch arguments, fixed at capture
        (`check_captured()` refuses a replay after they were edited); the grouped form reads all of them from its device
        table.  With skip_nonfinite there are three launches (_step_gated_guarded): the guard sits between the two, looks at
        `due` itself and gates the update by its own word, which it clears on a replay that is not due."""
        if self._cap_tags is None:
            raise RuntimeError("FlatAdamW.step_gated: call set_coverage() first")
        if self.skip_nonfinite:
            return self._step_gated_guarded(due, grad_clip)
        ema = self._ema_args() if self._ema_on else None
        if not torch.cuda.is_current_stream_capturing():
            self.sync_hyperparameters()
        n_p = ctypes.c_int32(0)
        flat = self.gb.flat
        check(lib().mesm_grad_sumsq_gated(ptr(flat), flat.numel(), ptr(self._cap_partials), ctypes.byref(n_p),
                                          ptr(self.step_t), ptr(due), stream_ptr()), "mesm_grad_sumsq_gated")
        clip = float(grad_clip or 0.0)
        clip = clip if clip > 0 else 0.0
        self.last_norm = self._cap_norm
        if self._stats_on:
            self._stats(due, self._stats_has_grad)
        if self._grouped:
            args = (ptr(self.flat_p), ptr(flat), ptr(self.exp_avg), ptr(self.exp_avg_sq), ptr(self._cap_tags),
                    self.flat_p.numel(), ptr(self._cap_partials), n_p.value, clip, ptr(self._table), len(self._step0),
                    ptr(self.step_t), ptr(self._cap_norm), ptr(due))
            if ema is not None:
                check(lib().mesm_adamw_step_groups_ema_gated(*args, *ema, stream_ptr()), "mesm_adamw_step_groups_ema_gated")
            else:
                check(lib().mesm_adamw_step_groups_gated(*args, stream_ptr()), "mesm_adamw_step_groups_gated")
            return
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        self._cap_baked = (float(b1), float(b2), float(g["eps"]), float(g["weight_decay"]))
        args = (ptr(self.flat_p), ptr(flat), ptr(self.exp_avg), ptr(self.exp_avg_sq), ptr(self._cap_tags),
                self.flat_p.numel(), ptr(self._cap_partials), n_p.value, clip, ptr(self.lr_t), *self._cap_baked,
                ptr(self.step_t), ptr(self._cap_norm), ptr(due))
        if ema is not None:
            check(lib().mesm_adamw_step_ema_gated(*args, *ema, stream_ptr()), "mesm_adamw_step_ema_gated")
        else:
            check(lib().mesm_adamw_step_gated(*args, stream_ptr()), "mesm_adamw_step_gated")

    def check_captured(self):
        """before a replay of a captured step_gated(): RuntimeError when the default form's by-value hyperparameters
        were edited since the capture (the replay would go on using the old ones), or inside swap_ema() (the update
        would train the average)"""
        if self._swapped:
            raise RuntimeError("FlatAdamW: no replay of a captured update inside swap_ema() (the parameters hold the average)")
        if self._cap_baked is not None:
            g = self.param_groups[0]
            now = (float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]))
            if now != self._cap_baked:
                raise RuntimeError("FlatAdamW: betas / eps / weight_decay of the default form are fixed in a captured update "
                                   "(%r at capture, %r now): capture again, or use parameter groups, whose hyperparameters "
                                   "all live in device memory" % (self._cap_baked, now))

    def zero_grad(self, set_to_none=True):
        self.model.zero_grad(set_to_none=set_to_none)

    # ------------------------------------------------------------------ checkpoints (torch.optim.AdamW format)
    def _members(self):
        """per group: [(parameter, offset)] in the group's own order -- torch numbers the parameters of a state dict
        through the groups in order"""
        return [[(p, self.gb.offsets[self._index[id(p)]]) for p in g["params"]] for g in self.param_groups]

    def state_dict(self):
        self._ensure()
        step = int(self.step_t.item())
        state, groups, i = {}, [], 0
        for g, members, step0 in zip(self.param_groups, self._members(), self._step0):
            for p, off in members:
                sl = slice(off, off + p.numel())
                v = self.exp_avg_sq[sl].view(p.shape).clone()
                if self._grouped:  # (the default form keeps writing the raw moment, as it always has)
                    v *= _v_scale(g["betas"][1], step - step0)
                state[i] = {"step": torch.tensor(float(step - step0)),
                            "exp_avg": self.exp_avg[sl].view(p.shape).clone(), "exp_avg_sq": v}
                i += 1
            out = {k: v for k, v in g.items() if k != "params"}
            out["params"] = list(range(i - len(members), i))
            groups.append(out)
        sd = {"state": state, "param_groups": groups}
        if self._ema_on:  # (torch.optim.AdamW.load_state_dict takes a dict with this extra key and drops it)
            src = self._ema_src()
            sd["ema"] = {"decay": self._ema_decay, "warmup": bool(self.ema_warmup), "num_updates": step - self._ema_step0,
                         "params": [src[off:off + p.numel()].view(p.shape).clone()
                                    for members in self._members() for p, off in members]}
        if self.skip_nonfinite:  # (an extra key like "ema")
            st = self._guard_state.tolist()
            sd["nonfinite"] = {"skipped": int(st[1]), "attempts": int(st[0])}
        return sd

    def load_state_dict(self, sd):
        self._ensure()
        saved = sd["param_groups"]
        members = self._members()
        if len(saved) != len(members):
            raise ValueError("loaded state dict has %d parameter groups, the optimizer has %d" % (len(saved), len(members)))
        for k, (sg, ms) in enumerate(zip(saved, members)):
            if len(sg["params"]) != len(ms):
                raise ValueError("loaded state dict's group %d has %d parameters, the optimizer's has %d"
                                 % (k, len(sg["params"]), len(ms)))
            if sg.get("amsgrad") or sg.get("maximize"):
                raise ValueError("FlatAdamW has no amsgrad / maximize (loaded group %d, which starts with %s)"
                                 % (k, self._name_of(ms[0][0])))
        group_step = []
        for sg, ms in zip(saved, members):
            step = 0
            for pid, (p, off) in zip(sg["params"], ms):
                st = sd["state"].get(pid)
                if st is None:
                    continue
                sl = slice(off, off + p.numel())
                self.exp_avg[sl].copy_(st["exp_avg"].reshape(-1))
                self.exp_avg_sq[sl].copy_(st["exp_avg_sq"].reshape(-1))
                if self._grouped:
                    self.exp_avg_sq[sl] /= _v_scale(sg.get("betas", self.defaults["betas"])[1], int(float(st["step"])))
                step = max(step, int(float(st["step"])))
            group_step.append(step)
        total = max(group_step)
        self.step_t.fill_(total)
        self._step0 = [total - s for s in group_step]
        for g, sg in zip(self.param_groups, saved):
            for k, v in sg.items():
                if k != "params":
                    g[k] = v
        self._hyper_host = None
        if self.skip_nonfinite:  # (without the flag a "nonfinite" key is ignored)
            # the two totals travel; the per-tensor counts describe the run that made them and start over
            saved_nf = sd.get("nonfinite") or {"skipped": 0, "attempts": 0}
            self._guard_state.copy_(torch.tensor([int(saved_nf["attempts"]), int(saved_nf["skipped"]), 0, 0],
                                                 dtype=torch.int32))
            self._guard_counts.zero_()
            self._guard_last = (int(saved_nf["skipped"]), np.zeros(len(self._guard_order), dtype=np.int64))
        if not self._ema_on:
            return  # (an "ema" key is ignored)
        saved_ema = sd.get("ema")
        if saved_ema is None:
            self.reset_ema()
            return
        flat_members = [m for ms in members for m in ms]
        if len(saved_ema["params"]) != len(flat_members):
            raise ValueError("loaded state dict's EMA has %d tensors, the optimizer covers %d"
                             % (len(saved_ema["params"]), len(flat_members)))
        dst = self._ema_src()
        for t, (p, off) in zip(saved_ema["params"], flat_members):
            dst[off:off + p.numel()].copy_(t.reshape(-1))
        self._ema_decay = _check_ema_decay(saved_ema["decay"])
        self.ema_warmup = bool(saved_ema["warmup"])
        self._ema_step0 = total - int(saved_ema["num_updates"])
        self._sync_ema()


def param_groups(model, rules=(), no_decay_1d=False, **defaults):
    """Torch-style group dicts over the trainable tensors of `model`, for FlatAdamW(model, params=...) or
    torch.optim.AdamW.

    rules: a sequence of (pattern, options).  `pattern` is a name prefix (str) or a compiled regex (`.search` on the
    named_parameters() name); the FIRST matching rule takes the tensor.  `options` holds any of lr, weight_decay,
    betas, eps, which override `defaults` for that group, or freeze=True: those tensors are left out of every group.
    Tensors no rule matches form the first group, with `defaults` alone.  With no_decay_1d, the tensors with
    ndim <= 1 (biases, LayerNorm, PReLU slopes) of each group move to a twin group right behind it with
    weight_decay = 0.  Empty groups are dropped."""
    known = set(_HYPER) | {"freeze"}
    for key in defaults:
        if key not in _HYPER:
            raise ValueError("unknown default %r (one of %s)" % (key, ", ".join(_HYPER)))
    rules = list(rules)
    for pattern, options in rules:
        if not isinstance(pattern, str) and not hasattr(pattern, "search"):
            raise ValueError("a rule's pattern is a name prefix or a compiled regex, not %r" % (pattern,))
        for key in options:
            if key not in known:
                raise ValueError("unknown option %r in the rule for %r (one of %s)"
                                 % (key, pattern, ", ".join(sorted(known))))
    buckets = [dict(defaults, params=[])]
    for _, options in rules:
        buckets.append(dict(defaults, params=[], **{k: v for k, v in options.items() if k != "freeze"}))
    gb = model.gradbuf()
    for name, p in zip(gb.names, gb.params):
        hit = next((r for r, (pattern, _) in enumerate(rules)
                    if (name.startswith(pattern) if isinstance(pattern, str) else pattern.search(name))), None)
        if hit is None:
            buckets[0]["params"].append(p)
        elif not rules[hit][1].get("freeze"):
            buckets[hit + 1]["params"].append(p)
    groups = []
    for b in buckets:
        if no_decay_1d:
            groups.append(dict(b, params=[p for p in b["params"] if p.ndim > 1]))
            groups.append(dict(b, params=[p for p in b["params"] if p.ndim <= 1], weight_decay=0.0))
        else:
            groups.append(b)
    return [g for g in groups if g["params"]]


def build_optimizer(opt, model):
    """runner.py:348-352 with the flat AdamW: (optimizer, StepLR scheduler)."""
    optimizer = FlatAdamW(model, lr=opt.lr, weight_decay=opt.weight_decay, ema_decay=getattr(opt, "ema_decay", None),
                          ema_warmup=getattr(opt, "ema_warmup", False),
                          skip_nonfinite=getattr(opt, "skip_nonfinite", False),
                          tensor_stats=getattr(opt, "tensor_stats", None))
    lr_scheduler = torch.optim.lr_scheduler.StepLR(optimizer, opt.lr_drop, gamma=opt.gamma)
    return optimizer, lr_scheduler
