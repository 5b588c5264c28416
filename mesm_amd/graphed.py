"""A whole training step (forward + criterion + backward [+ gradient all-reduce]) captured in ONE
HIP graph, and a cache of such graphs keyed by batch shape.

The eager path issues ~700 kernel launches per step from Python and is host-bound; for a fixed
batch *shape* every launch argument is static, so the step is captured once
(torch.cuda.CUDAGraph records the HIP launches our C-ABI makes on the capture stream) and
replayed with a single host call.  What stays dynamic is moved to device memory:

  * the batch tensors are static buffers, refreshed with `load_batch()`;
  * every data-dependent host decision of the forward and of the criterion (group gathers, GT-clip
    gathers, flattened targets, rec_ss positives: model.Plan / criterion.TargetPlan) lives in static
    index tensors that `load_batch()` REBUILDS from the new batch on the host and copies over; their
    data-dependent extents (GT clips per pair Lc, group video length Lss, target windows) are padded
    to capture-time capacities, and a batch that does not fit raises ValueError (StepCache then
    captures another graph);
  * the host-RNG draws of the reference (negative query index, masked-LM word choice) are
    static index tensors, refreshed with `redraw()` before each replay;
  * dropout seeds: the kernels add a device-side counter (`seed_offset`) that the graph itself
    increments at the start of every replay, so each step gets fresh masks.

Gradients land in the model's flat gradient buffer (param.grad aliases it), exactly as in the
eager path, so optimizer / clip_grad_norm_ work unchanged after `run()`.  With a `reducer`
(ddp.GradReducer) the bucketed gradient all-reduce is captured INSIDE the graph on the process
group's side stream: bucket k reduces while the rest of backward runs.

The captured launches bake in the addresses of the parameters: they must not move afterwards.
`build_model` / `FlatAdamW.__init__` flatten the parameters eagerly (model.flat_params), and `run()`
raises if an address differs from capture time.
"""
import os
from collections import OrderedDict

import torch

from . import draws
from . import kernels as kn
from .batching import bucket_key, shape_batch
from .criterion import TargetPlan, loss_pack


def map_tree(fn, tree):
    """{k: fn(k, v)} over a batch or an output dict, into its lists of dicts (per-pair targets, aux_outputs): fn(inner key,
    value) there.  fn sees every value, tensor or not."""
    return {k: ([{kk: fn(kk, vv) for kk, vv in d.items()} for d in v] if isinstance(v, list) and v and isinstance(v[0], dict)
                else fn(k, v)) for k, v in tree.items()}


def capture_batch(batch, device):
    """the capture's own copy of a shaped batch: every tensor copied to `device` (words_weight stays where it is, as
    prepare_batch_input leaves it; a tensor already there is cloned); the big feature tensors of a pair-padded batch, which
    keep their real rows only (batching.pad_pairs), padded to the pair extent on the device"""
    def copy(k, v):
        if not torch.is_tensor(v):
            return v
        return v.clone() if k == "words_weight" else v.to(device, copy=True)
    static = map_tree(copy, batch)
    if "_n_real" in batch:
        P = static["video_mask"].shape[0]
        for k in ("video_feat", "words_id"):
            t = static[k]
            if t.shape[0] < P:
                static[k] = torch.cat([t, t[:1].expand((P - t.shape[0],) + tuple(t.shape[1:]))]).contiguous()
    return static


_CAPTURE_STREAMS = {}


def capture_stream(dev):
    """THE stream of this process on which steps are warmed up and captured (one per device).  Autograd pins an
    AccumulateGrad node to the stream of its first use for as long as the node lives, and the graph of a warm-up step
    can live on through reference cycles; a later capture on ANOTHER stream records the hand-over to that stream as a
    side branch of the HIP graph -- a second hardware queue at replay, +0.3 ms per step.  With one stream for every
    warm-up and capture of the process there is nothing to hand over, however many graphs are captured."""
    key = torch.device(dev).index if torch.device(dev).index is not None else torch.cuda.current_device()
    st = _CAPTURE_STREAMS.get(key)
    if st is None:
        st = _CAPTURE_STREAMS[key] = torch.cuda.Stream(device=dev)
    return st


class _DrawRing:
    """The per-step host draws reach the device through a ring of pinned host buffers that the FIRST NODE of the
    captured step reads itself (kernels.step_begin), instead of a host-to-device copy between two replays: replay n
    reads slot n % SLOTS -- the device counts its own replays -- so the host publishes the draws of replay n into that
    slot right before launching it and waits, when it gets SLOTS - 1 replays ahead, for the replay that last used the
    slot."""
    SLOTS = 4

    def __init__(self, arena, names, device):
        self.arena = arena
        self.lo, self.hi = arena.span(names)
        self.nbytes = self.hi - self.lo
        self.ring = torch.zeros(self.SLOTS * self.nbytes, dtype=torch.uint8).pin_memory()
        self.host = self.ring.numpy()
        self.ctr = torch.zeros(1, dtype=torch.int32, device=device)
        self.dst = arena.dev[self.lo:self.hi]
        self.n = 0
        self.events = [None] * self.SLOTS

    def capture_node(self, seed_ctr):
        kn.step_begin(self.ring, self.nbytes, self.SLOTS, self.dst, self.ctr, seed_ctr)

    def publish(self, arrays):
        s = self.n % self.SLOTS
        if self.events[s] is not None:
            self.events[s].synchronize()  # the replay SLOTS launches ago has read this slot
        self.arena.pack(arrays, self.lo, self.hi, self.host[s * self.nbytes:(s + 1) * self.nbytes])
        return s

    def launched(self, s):
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self.events[s] = ev
        self.n += 1


class _PulledGraph:
    """graph.replay() that first publishes the owner's current draws for the replay's first node"""

    def __init__(self, graph, owner):
        self._g, self._o = graph, owner

    def replay(self):
        o = self._o
        s = o._pull.publish(o._arr)
        self._g.replay()
        o._pull.launched(s)

    def __getattr__(self, k):
        return getattr(self._g, k)


class GraphedStep:
    BIG = 1 << 20  # batch tensors above 1 MiB (video_feat, word features) are copied on their own
    DRAWN = ("p.neg_index", "p.masked_words")  # what redraw() changes: the host RNG draws of a step
    TRAIN = True     # a training step (EvalGraphedStep: a forward-only evaluation step)
    _targets = True  # the arena holds the criterion's target plan

    def __init__(self, model, criterion, batch, dataset_name, warmup=3, instrument=False, reducer=None,
                 caps=None, group_cap=None, micro_steps=None, optimizer=None, grad_clip=0.0):
        """caps: None = exact extents of `batch` (benchmarks); "auto" = bucketed capacities so that other
        batches of the same (N, Lv, Lw, groups) replay; or a dict with any of Lc / Lss / T / Tmax.
        micro_steps=k: k consecutive replays (of this graph or of other micro-stepped graphs of the model) form one cycle
        whose gradient is the MEAN of the k micro-batch gradients -- what k data-parallel ranks reduce to: the graph clears
        the flat gradient buffer on the first replay of a cycle only and seeds its backward with 1 / k; `update_due` is
        True after the k-th.  optimizer= (a FlatAdamW over this model; needs micro_steps, k = 1 allowed) also captures
        clip + AdamW update behind the backward; they act on the last replay of a cycle only (micro-batched steps)."""
        from .arena import Arena
        from .hostplan import HostSpec
        self._cycle = None
        self.optimizer, self.grad_clip = optimizer, float(grad_clip or 0.0)
        self._check_micro_args(model, reducer, micro_steps, optimizer)
        self.model, self.crit = model, criterion
        self.dataset_name = dataset_name
        self.spec = HostSpec.from_model(model, criterion, dataset_name)
        # the model's text cache (model.text_cache) is part of what the step is captured for: with it the graph holds
        # mesm_text_pool_slots over the static slot array p.text_slots and no tower; None = captured without
        self._tc = model._active_text_cache()
        dev = batch["video_feat"].device
        self.dev = dev
        self.batch = dict(batch)  # static inputs: big tensors as given, everything small re-homed in the arena
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self._seed = {}
        self.reducer = reducer
        # the step is captured in the model's CURRENT mode (train(): dropout on, fresh masks every replay;
        # eval(): dropout off, e.g. to reproduce a recorded step) -- like the reference's loop, which calls
        # model.train() itself (train.py:53)
        model.flat_params()
        self._groups = [int(g) for g in batch["num_clips"].tolist()]
        # batches padded to a pair capacity (batching.pad_pairs): the number of REAL pairs is a device scalar of the
        # captured step; None = the step was captured for exactly its pairs and stays that way
        self._n_real = batch.get("_n_real")
        self.batch.pop("_n_real", None)
        self.caps = self._resolve_caps(caps, batch, group_cap)
        # ONE device arena for: the forward's index plan, the criterion's target plan and the small batch tensors
        host = {k: v.detach().cpu() for k, v in batch.items() if torch.is_tensor(v)}
        for k in ("norm_span", "norm_moment"):
            if isinstance(batch.get(k), list):
                host[k] = [{kk: vv.detach().cpu() for kk, vv in d.items()} for d in batch[k]]
        arr, self._pmeta, self._tmeta, self._wm_cpu = self._host_arrays(host, None, None)
        text_miss = self._text_lookup(arr)
        self._arr = arr  # host mirror of the arena
        self._draws = (arr["p.neg_index"], arr.get("p.masked_words"))
        self.arena = Arena(arr, dev, first=self.DRAWN)  # the per-step draws sit together at the front
        # MESM_STEP_PULL=1: the draws are pulled from a pinned ring by the graph's first node instead of travelling as a
        # host-to-device copy between replays.  Measured equal (bench 3.964 vs 3.966 ms/step, profiles/r4c/
        # step_pull_ab.txt: the copy between two replays was never the 50 us tools/host_cost.py's 30-step loop
        # suggested), so the plain copy stays the default.
        self._pull = (_DrawRing(self.arena, self.DRAWN, dev)
                      if dev.type == "cuda" and os.environ.get("MESM_STEP_PULL", "0") == "1" else None)
        if micro_steps is not None:
            self._pull = None  # (a micro-stepped graph has its own first node: the draws travel as the plain copy)
        v = self.arena.views
        self.plan = model.plan_from({k[2:]: t for k, t in v.items() if k.startswith("p.")}, self._pmeta)
        self.tplan = None
        if self._tmeta is not None:
            self.tplan = TargetPlan.__new__(TargetPlan)
            self.tplan.adopt({k[2:]: t for k, t in v.items() if k.startswith("t.")}, self._tmeta)
        for k, t in v.items():
            if k.startswith("b."):
                self.batch[k[2:]] = t
        if self.tplan is not None:
            self.batch["_target_plan"] = self.tplan
        if self._n_real is not None:
            self.batch["_n_valid"] = v["p.n_valid"]
        # the capture batch's misses, in front of the warm-up passes (which read the slots like a replay does and count
        # nothing in the cache's stats)
        self._text_encode(text_miss)
        gb = model.gradbuf()
        gb.ensure(dev)
        saved_state = None
        if micro_steps is not None:
            self._cycle = gb.cycle_state(dev)
            self._cycle.set_k(micro_steps)
            # the warm-up steps and the capture run real backward passes (and updates): what a cycle under way has
            # accumulated, the cycle words, the parameters and the optimizer state come out of them unchanged
            saved_state = self._save_training_state()
        kn.set_seed_offset(self.counter)
        try:
            side = capture_stream(dev)
            # autograd graphs of earlier (eager) steps can live on through reference cycles and keep their
            # AccumulateGrad nodes -- pinned to the stream THEY ran on -- alive: collect them before the first warm-up
            import gc
            gc.collect()
            side.wait_stream(torch.cuda.current_stream())
            # A reducer learns its bucket schedule on its first step, so the first graph warms up with the
            # collectives live (every rank is there together).  Later graphs of a StepCache are captured whenever
            # a rank meets a new batch shape -- not at the same step on every rank -- so their warm-up steps must
            # not issue collectives the other ranks do not match: the gradient hooks are detached for them.
            learnt = reducer is not None and getattr(reducer, "expected", None) is not None
            saved_hook = gb.on_ready
            if learnt:
                gb.on_ready = None
            try:
                with torch.cuda.stream(side):
                    for _ in range(max(warmup, 2 if (reducer is not None and not learnt) else 1)):
                        self._step_body()
                        if self._cycle is not None:
                            self._tail()
            finally:
                gb.on_ready = saved_hook
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            dot = os.environ.get("MESM_GRAPH_DOT")
            if dot:
                self.graph.enable_debug_mode()
            if self.TRAIN:
                model.zero_grad(set_to_none=True)
            if instrument:  # record the GEMM launches of the captured step (bench roofline)
                kn.gemm_tape(True)
            # capture_error_mode="thread_local": the process group's watchdog THREAD polls the events of earlier
            # (eager, warm-up) collectives whenever it likes; under the default global mode such a query during
            # our capture is an error that kills the process (seen in ~1 of 3 runs of the 1-rank RCCL test)
            # captured on the SAME stream the warm-up steps ran on: autograd pins every AccumulateGrad node (kept
            # alive by gradbuf's hooks) to the stream of its first use, and a capture on another stream records the
            # hand-over to that stream as a side branch of the graph -- a second hardware queue at replay, which
            # costs every kernel boundary of the main chain (5.2 -> 5.5 ms per step)
            self._capture(side)
            if dot:
                self.graph.debug_dump(dot)
            if self._pull is not None:
                self.graph = _PulledGraph(self.graph, self)
        finally:
            kn.set_seed_offset(None)
            if instrument:
                kn.gemm_tape(False)
            if saved_state is not None:
                self._restore_training_state(saved_state)
        self._ptrs = self._param_ptrs()

    def _capture(self, side):
        """the whole step -- forward, criterion, backward -- as ONE graph (SplitGraphedStep: three)"""
        with torch.cuda.graph(self.graph, stream=side, capture_error_mode="thread_local"):
            if self._cycle is not None:
                kn.micro_begin(self._cycle.words, self.counter)  # cycle position + seed offset += 1: one node
            elif self._pull is not None:
                self._pull.capture_node(self.counter)  # draws from the pinned ring + seed offset += 1: one node
            else:
                self.counter.add_(1)
            self.total, self.losses = self._step_body()
            if self._cycle is not None:
                self._tail()

    # ------------------------------------------------------------------ micro-batched replays (micro_steps=k)
    def _check_micro_args(self, model, reducer, micro_steps, optimizer):
        if micro_steps is None:
            if optimizer is not None:
                raise ValueError("%s: optimizer= captures the update of a micro-step cycle and needs micro_steps "
                                 "(micro_steps=1 updates at every replay)" % type(self).__name__)
            return
        if not self.TRAIN:
            raise ValueError("%s: micro_steps belongs to training steps" % type(self).__name__)
        if int(micro_steps) < 1:
            raise ValueError("micro_steps must be >= 1, got %r" % (micro_steps,))
        if reducer is not None:
            raise ValueError("%s: micro_steps together with reducer= is not supported: the collectives captured in the "
                             "step graph cannot be gated by the cycle" % type(self).__name__)
        if optimizer is not None:
            from .optim import FlatAdamW
            if not isinstance(optimizer, FlatAdamW):
                raise ValueError("optimizer= takes a mesm_amd.optim.FlatAdamW (its update runs on the flat buffers), not %s"
                                 % type(optimizer).__name__)
            if optimizer.gb is not model.gradbuf() or optimizer.flat_p is None or optimizer.flat_p is not model.flat_params():
                raise ValueError("optimizer= does not cover this model's flat buffers (it was built over another model, or "
                                 "the parameters were flattened again after it was built)")

    def _save_training_state(self):
        gb = self.model.gradbuf()
        torch.cuda.synchronize()
        st = {"flat": gb.flat.clone(), "words": self._cycle.words.clone()}
        opt = self.optimizer
        if opt is not None:
            # host edits of the hyperparameters reach the device BEFORE the snapshot: the warm-up passes would upload them
            # after it, and the restore would put the old device words back under a host that believes them current
            opt.sync_hyperparameters()
            # (with a weight EMA: the average, its decay words and the decay of the last update as well; with the non-finite
            # guard: its counters and `go` word, so that the warm-up passes leave no attempt behind; with per-tensor
            # statistics: the sample count and the result tables, so that a capture takes no sample)
            st["opt"] = [(t, t.clone()) for t in [opt.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.step_t] + opt.ema_tensors()
                         + opt.guard_tensors() + opt.tensor_stat_tensors()]
            st["norm"] = opt._cap_norm.clone() if opt._cap_norm is not None else None
        return st

    def _restore_training_state(self, st):
        gb = self.model.gradbuf()
        cyc = self._cycle
        torch.cuda.synchronize()
        gb.flat.copy_(st["flat"])
        cyc.words.copy_(st["words"])
        for t, saved in st.get("opt", ()):
            t.copy_(saved)
        if st.get("norm") is not None:
            self.optimizer._cap_norm.copy_(st["norm"])
        # .grad of every tensor that some micro-stepped graph of the model writes aliases its view (the gradients of a
        # cycle may come from several graphs): the same set after every capture, and what FlatAdamW.step() looks at
        mine = [p.grad is not None for p in gb.params]
        cyc.covered = [a or b for a, b in zip(cyc.covered, mine)] if cyc.covered is not None else mine
        for p, on in zip(gb.params, cyc.covered):
            p.grad = p._mesm_gview if on else None
        torch.cuda.synchronize()

    def _tail(self):
        """behind the backward of a micro-stepped step: clip + AdamW update of the captured optimizer, gated by the
        cycle's `due` word.  Outside a capture (warm-up) the coverage -- the tensors some graph of the model writes a
        gradient for -- is brought up to date first (a host-to-device copy into the same mask tensor)."""
        opt = self.optimizer
        if opt is None:
            return
        gb, cyc = self.model.gradbuf(), self._cycle
        mine = [p.grad is not None for p in gb.params]
        union = [a or b for a, b in zip(cyc.covered, mine)] if cyc.covered is not None else mine
        if torch.cuda.is_current_stream_capturing():
            if union != cyc.covered:
                raise RuntimeError("GraphedStep: the captured step writes gradients its warm-up step did not")
        elif union != cyc.covered or opt._cap_tags is None:
            cyc.covered = union
            opt.set_coverage(union)
        opt.step_gated(cyc.due_word, self.grad_clip)

    def _extra_ptrs(self):
        if self._cycle is None:
            return []
        extra = [self._cycle.words.data_ptr(), self._cycle.seed.data_ptr()]
        if self.optimizer is not None:
            extra += self.optimizer.captured_ptrs()
        return extra

    @property
    def micro_steps(self):
        return self._cycle.k if self._cycle is not None else None

    @property
    def update_due(self):
        """after run(): that replay was the last of its cycle -- the buffer holds the mean gradient (and, with a captured
        optimizer, the parameters have just been updated)"""
        return self._cycle is not None and self._cycle.due

    @property
    def updates(self):
        return self._cycle.updates if self._cycle is not None else 0

    def set_micro_steps(self, k):
        """another k from the next cycle on, without a new capture (k is a device word, the backward seed a tensor);
        RuntimeError in the middle of a cycle"""
        if self._cycle is None:
            raise RuntimeError("%s was captured without micro_steps" % type(self).__name__)
        self._cycle.set_k(k)

    def reset_cycle(self):
        """drop an unfinished cycle (the ragged end of an epoch): the next replay clears the gradient buffer"""
        if self._cycle is None:
            raise RuntimeError("%s was captured without micro_steps" % type(self).__name__)
        self._cycle.reset()

    # ------------------------------------------------------------------ host half (shared with the loader workers)
    def _resolve_caps(self, caps, batch, group_cap=None):
        return self.spec.resolve_caps(caps, batch, self._groups, group_cap)

    def _host_arrays(self, host, neg_index, masked_words, targets=True):
        """hostplan.HostSpec.host_arrays with this step's groups / capacities: {name: numpy array} of everything small
        the captured step reads, the two metas and the word mask"""
        arr, pmeta, tmeta, wm = self.spec.host_arrays(host, self._groups, self.caps, self._n_real, neg_index, masked_words,
                                                      self.BIG, targets=targets and self._targets, is_training=self.TRAIN)
        return self._with_text_slots(arr), pmeta, tmeta, wm

    # ------------------------------------------------------------------ text cache (model.text_cache, textcache.py)
    def _with_text_slots(self, arr):
        """`arr` with the plan entry p.text_slots (int32 per pair, zeros until _text_lookup) in front of the criterion's
        arrays, which stay together at the end of the arena; `arr` itself without a text cache"""
        if self._tc is None:
            return arr
        import numpy as np
        if "b.words_id" not in arr or arr["b.words_id"].ndim != 2:
            raise ValueError("%s: the text cache needs the batch's token ids (N, context_length) on the host"
                             % type(self).__name__)
        out = {}
        for k, v in arr.items():
            if k.startswith("t."):
                out.setdefault("p.text_slots", np.zeros(arr["p.vpad"].shape[0], dtype=np.int32))
            out[k] = v
        out.setdefault("p.text_slots", np.zeros(arr["p.vpad"].shape[0], dtype=np.int32))
        return out

    def _text_lookup(self, arr):
        """the slots of the batch's queries into arr["p.text_slots"] (padding pairs are copies of pair 0: its key, its
        slot) -> the misses, to be encoded by _text_encode once the batch's ids are on the device.  ValueError (more
        distinct queries than slots) before anything changes; call it after every other check."""
        if self._tc is None:
            return None
        import numpy as np
        if self._text_pending:
            self._tc.clear()  # (a load that failed between its lookup and its fill: the table names unwritten slots)
        ids, P = arr["b.words_id"], arr["p.text_slots"].shape[0]
        if ids.shape[0] < P:
            ids = np.concatenate([ids, np.repeat(ids[:1], P - ids.shape[0], axis=0)])
        slots, rows, dst = self._tc.lookup(ids, self.model.text_encoder.weights_generation)
        arr["p.text_slots"] = slots
        self._text_pending = bool(rows)
        return rows, dst

    _text_pending = False

    def _text_encode(self, miss):
        """the tower on the loaded batch's missing queries, eagerly on the current stream -- the one the replay runs on,
        so a rewritten slot stays behind every earlier reader"""
        if self._tc is None:
            return
        try:
            self.model.text_cache_encode(self._tc, self.batch["words_id"], miss[0], miss[1])  # (empties the table if it fails)
        finally:
            self._text_pending = False
            self._tc_version = self._tc.version

    def _check_text_cache(self):
        """before a replay: the switch is what the step was captured for (RuntimeError otherwise: load_batch says it with
        a ValueError, which sends a cache to another graph); and when the cache's table changed since this step's batch
        was loaded -- another step's batch, an invalidation -- the loaded batch is looked up (and encoded) again"""
        tc = self._tc
        if tc is None and self.model._text_cache_req is None:
            return
        if self.model._active_text_cache() is not tc:
            raise RuntimeError("%s: the model's text cache was switched %s after capture; capture again"
                               % (type(self).__name__, "off or replaced" if tc is not None else "on"))
        if tc is not None and (tc.version != self._tc_version
                               or tc._source_gen != self.model.text_encoder.weights_generation):
            miss = self._text_lookup(self._arr)
            self.arena.upload(self._arr, only=["p.text_slots"])
            self._text_encode(miss)

    def _param_ptrs(self):
        gb = self.model.gradbuf()
        return [p.data_ptr() for p in gb.params] + [gb.flat.data_ptr()] + self._extra_ptrs()

    def _step_body(self):
        b = self.batch
        out = self.model(**b, dataset_name=self.dataset_name, is_training=True, plan=self.plan)
        losses, total = self.crit(out, b, True)
        self.model.zero_grad(set_to_none=True)
        # a hooked reducer launches its bucket collectives from inside and joins at the end; with fold_scale the
        # 1 / world of the gradient MEAN rides the loss gradient (one scalar) instead of a pass over the flat buffer
        sc = self.reducer.backward_scale() if self.reducer is not None else 1.0
        if self._cycle is not None:
            # 1 / k of the gradient MEAN rides the loss gradient, from the cycle's own tensor (set_micro_steps refills it);
            # the clear of the flat buffer is gated by the cycle's phase and plain-autograd gradients are added to it
            gb = self.model.gradbuf()
            gb.gated = self._cycle
            try:
                total.backward(self._cycle.seed.view(total.shape))
            finally:
                gb.gated = None
            return total.detach(), {k: v.detach() for k, v in losses.items()}
        # the seed of the backward pass from a tensor made once (autograd's own ones_like is a fill launch per step)
        seed = self._seed.get(sc)
        if seed is None or seed.shape != total.shape:
            seed = self._seed[sc] = torch.full_like(total, sc)
        total.backward(seed)
        return total.detach(), {k: v.detach() for k, v in losses.items()}

    # ------------------------------------------------------------------ new batch, same graph
    def load_batch(self, batch, redraw=False, host=None, defer_targets=False):
        """Make the captured step run on `batch` (host tensors; device tensors are brought to the host first,
        the plans are host work): same (N, Lv, Lw, Dv, Dt) and the same group sizes; GT-clip counts, group video
        lengths and target windows may differ within the capture-time capacities.  Everything small -- index
        plans, targets, masks, labels -- goes up in ONE pinned transfer (arena.Arena), the feature tensors in one
        copy each.  redraw: also draw new negatives / MLM words here (then call run(redraw=False): one upload per
        step instead of two).  Raises ValueError (nothing is modified) when it does not fit."""
        groups = [int(g) for g in (batch if host is None else host)["num_clips"].tolist()]
        n_real = batch.get("_n_real")
        self._check_fits(groups, n_real)
        old_groups, self._groups = self._groups, groups
        old_real, self._n_real = self._n_real, n_real
        try:
            self._load_batch(batch, redraw, host, defer_targets)
        except ValueError:
            self._groups, self._n_real = old_groups, old_real
            raise

    def _load_batch(self, batch, redraw, host_given=None, defer_targets=False):
        for k, cur in self.batch.items():
            v = batch.get(k)
            if k == "num_clips" or k.startswith("_"):
                continue
            if k == "video_feat" and torch.is_tensor(v) and v.dtype != cur.dtype:
                # (copy_ would convert on the way into the static input: a float16 batch wants a graph of its own)
                raise ValueError("GraphedStep.load_batch: video_feat changed dtype %s -> %s" % (cur.dtype, v.dtype))
            if torch.is_tensor(cur) and torch.is_tensor(v) and cur.shape != v.shape:
                if k in ("video_feat", "words_id") and cur.shape[1:] == v.shape[1:] and v.shape[0] <= cur.shape[0] \
                        and self._n_real is not None:
                    continue  # the real rows only: the rest of the static input keeps (finite) older rows
                raise ValueError("GraphedStep.load_batch: %s changed shape %s -> %s"
                                 % (k, tuple(cur.shape), tuple(v.shape)))
        if host_given is not None:
            # (autograph._Fetch: every small tensor of a device batch in ONE transfer, the word mask formed on the device)
            host = {k: v for k, v in host_given.items() if torch.is_tensor(v) or isinstance(v, list)}
        else:
            host = {k: (v.detach().cpu() if v.is_cuda and v.numel() * v.element_size() <= self.BIG else v)
                    for k, v in batch.items() if torch.is_tensor(v)}
            for k in ("video_mask", "clip_mask"):
                if k in host and host[k].is_cuda:
                    host[k] = host[k].cpu()
            if host["words_id"].is_cuda:
                host["words_id"] = host["words_id"].cpu()
            for k in ("norm_span", "norm_moment"):
                if isinstance(batch.get(k), list):
                    host[k] = [{kk: vv.detach().cpu() for kk, vv in d.items()} for d in batch[k]]
        # keep the current host draws unless asked to redraw (plan_arrays draws when given None)
        arr, pmeta, tmeta, wm = self._host_arrays(host, None if redraw else self._draws[0],
                                                  None if redraw else self._draws[1], targets=not defer_targets)
        if defer_targets:
            # the criterion's arrays are built and uploaded by finish_targets(), after the forward graph has been launched;
            # until then the arena image keeps the previous batch's (they are not part of this upload)
            arr.update({k: v for k, v in self._arr.items() if k.startswith("t.")})
            self._pending_targets = host
        self._check_fits(self._groups, self._n_real, pmeta)  # (groups and pair count: checked by load_batch)
        self.arena.check(arr)
        text_miss = self._text_lookup(arr)
        # nothing above modified anything; from here on only copies
        self._arr = arr
        self._draws = (arr["p.neg_index"], arr.get("p.masked_words"))
        if defer_targets:
            self.arena.upload(arr, only=[k for k in arr if not k.startswith("t.")])
        else:
            self.arena.upload(arr)
            if tmeta is not None:
                self.tplan.sizes, self.tplan.sumT = tmeta["sizes"], tmeta["sumT"]
        for k, cur in self.batch.items():
            v = batch.get(k)
            if k.startswith("_"):
                continue
            if k == "num_clips":
                self.batch[k] = v  # host-side bookkeeping only (the step reads the plans)
                continue
            if torch.is_tensor(cur) and torch.is_tensor(v) and ("b." + k) not in arr:
                if not cur.is_cuda:
                    self.batch[k] = v  # host-side inputs (words_weight) are only read by redraw()
                elif v.is_cuda:
                    cur[:v.shape[0]].copy_(v, non_blocking=True)
                else:
                    self._stage_big(k, cur, v)
        self._text_encode(text_miss)
        self._turn ^= 1
        self._wm_cpu = wm

    _pending_targets = None

    def _check_fits(self, groups, n_real, pmeta=None):
        """ValueError unless a batch of these group sizes, this pair-count mode and (given) this plan meta fits the graph"""
        if self.model._active_text_cache() is not self._tc:
            raise ValueError("%s: captured %s the model's current text cache" % (type(self).__name__,
                                                                               "without" if self._tc is None else "with another than"))
        if groups != self._groups and (self.caps.get("M") is None or sum(groups) != sum(self._groups)):
            # exact-extent graphs (caps=None) are tied to their grouping; with capacities any grouping of the
            # same number of pairs fits as long as its largest group does (checked by the plan)
            raise ValueError("%s: group sizes changed %s -> %s" % (type(self).__name__, self._groups, groups))
        if (n_real is None) != (self._n_real is None):
            raise ValueError("%s: the step was captured %s a device-side pair count"
                             % (type(self).__name__, "with" if self._n_real is not None else "without"))
        for k in ("vid_identity", "has_vid_src"):
            if pmeta is not None and pmeta.get(k) != self._pmeta.get(k):
                raise ValueError("%s: plan.%s changed (%r -> %r): needs its own graph"
                                 % (type(self).__name__, k, self._pmeta.get(k), pmeta.get(k)))

    def finish_targets(self):
        """second half of load_batch(defer_targets=True): the criterion's flattened targets, built and uploaded while the
        forward graph runs.  Raises ValueError when they do not fit the captured capacities (the caller then runs the step
        eagerly: nothing but static graph memory has been touched)."""
        host, self._pending_targets = self._pending_targets, None
        tarr, tmeta = self.spec.target_arrays(host, self.caps)
        arr = dict(self._arr)
        arr.update(tarr)
        self.arena.check(arr)
        self._arr = arr
        self.arena.upload(arr, only=list(tarr))
        self.tplan.sizes, self.tplan.sumT = tmeta["sizes"], tmeta["sumT"]

    def load_prepared(self, prep):
        """load_batch for a batch whose host half was done elsewhere (loader.HostPipeline.prepare in a worker process):
        `prep` carries the arena arrays (placeholder draws), the metas, the word mask and the big feature tensors
        (pinned when they came through a DataLoader with pin_memory).  Here: compatibility checks, the two host-RNG
        draws of the reference's forward (in THIS process: its RNG stream), one arena upload, the feature copies.
        Raises ValueError (nothing modified) when the batch does not fit this graph."""
        if prep["spec"] != self.spec:
            raise ValueError("GraphedStep.load_prepared: prepared for another model configuration")
        groups = prep["groups"]
        self._check_fits(groups, prep["n_real"], prep["pmeta"])
        if {k: prep["caps"].get(k) for k in self.caps} != self.caps:
            raise ValueError("GraphedStep.load_prepared: prepared with other capacities %r (graph: %r)" % (prep["caps"], self.caps))
        arr = self._with_text_slots({k: (v.numpy() if torch.is_tensor(v) else v) for k, v in prep["arr"].items()})
        self.arena.check(arr)
        big = prep["big"]
        for k, v in big.items():
            cur = self.batch[k]
            if v.dtype != cur.dtype:
                raise ValueError("GraphedStep.load_prepared: %s changed dtype %s -> %s" % (k, cur.dtype, v.dtype))
            # fewer rows than the static input only where the step reads the real pair count from the device (like
            # load_batch: without it the stale rows of the previous batch would take part in the step)
            if cur.shape[1:] != v.shape[1:] or v.shape[0] > cur.shape[0] or (v.shape[0] < cur.shape[0] and self._n_real is None):
                raise ValueError("GraphedStep.load_prepared: %s changed shape %s -> %s" % (k, tuple(cur.shape), tuple(v.shape)))
        text_miss = self._text_lookup(arr)  # (the table lives in this process: workers know no model)
        # nothing above modified anything; from here on: draws, copies
        self._groups, self._n_real = groups, prep["n_real"]
        self._wm_cpu = prep["wm"]
        self.batch["words_weight"] = prep["words_weight"]
        self.batch["num_clips"] = prep["num_clips"]
        neg = draws.neg_index(self._groups, self._n_real)
        arr["p.neg_index"] = neg
        mw = None
        if "p.masked_words" in arr:
            mw = draws.masked_words(self._wm_cpu, prep["words_weight"])
            arr["p.masked_words"] = mw
        self._arr, self._draws = arr, (neg, mw)
        self.arena.upload(arr)
        self.tplan.sizes, self.tplan.sumT = prep["tmeta"]["sizes"], prep["tmeta"]["sumT"]
        for k, v in big.items():
            self._stage_big(k, self.batch[k], v)
        self._text_encode(text_miss)
        self._turn ^= 1

    _copy_stream = None
    _turn = 0

    def _stage_big(self, k, cur, v):
        """host feature tensor -> static graph input without stalling the compute stream: the (pageable, hence
        host-blocking) H2D runs on a copy stream into one of two device staging buffers while the previous
        replay is still executing; the compute stream then only does a device-to-device copy (27 MB: ~10 us)
        behind an event.  A staging buffer is rewritten only after the D2D copy that read it two batches ago."""
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=self.dev)
            self._stages, self._d2d_done = {}, {}
        j = self._turn
        st = self._stages.setdefault(k, [None, None])
        if st[j] is None:
            st[j] = torch.empty_like(cur)
        main, cs = torch.cuda.current_stream(), self._copy_stream
        n = v.shape[0]  # (fewer rows than the static input: a padded batch's real pairs)
        with torch.cuda.stream(cs):
            ev = self._d2d_done.get((k, j))
            if ev is not None:
                cs.wait_event(ev)
            st[j][:n].copy_(v, non_blocking=True)
            done = torch.cuda.Event()
            done.record(cs)
            from .loader import H2D_EVENTS
            H2D_EVENTS.append(done)  # (a ring slot of loader.PinnedRing is rewritten only after the copy that read it)
        main.wait_event(done)
        cur[:n].copy_(st[j][:n], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(main)
        self._d2d_done[(k, j)] = ev

    def redraw(self):
        """New negative-query indices and MLM word choices (host RNG, like the reference does on every forward),
        written into the static index tensors the graph reads (one arena upload)."""
        m = self.model
        neg = draws.neg_index(self._groups, self._n_real)
        mw = None
        if hasattr(self.plan, "masked_words"):
            mw = draws.masked_words(self._wm_cpu, self.batch["words_weight"])
        self._draws = (neg, mw)
        self._arr["p.neg_index"] = neg
        if mw is not None:
            self._arr["p.masked_words"] = mw
        if self._pull is None:
            self.arena.upload(self._arr, only=self.DRAWN)  # ~1 KB instead of the whole 57 KB arena
        # (with the ring: the next replay publishes self._arr's draws itself)

    def set_draws(self, neg_index, masked_words=None):
        """replay with given host draws (tests / reproducing a recorded step)"""
        neg = neg_index.cpu().numpy()
        mw = masked_words.cpu().numpy().astype(bool) if masked_words is not None else self._draws[1]
        self._draws = (neg, mw)
        self._arr["p.neg_index"] = neg
        if mw is not None:
            self._arr["p.masked_words"] = mw
        self.arena.upload(self._arr)

    def _check_addresses(self):
        """the address comparison of run() (273 addresses: 0.1 ms of the caller's critical path) only when the model says
        tensors may have moved (MESM._apply / a re-flattening bump _addr_gen); the two flat buffers' addresses every time"""
        m = self.model
        gen = m.__dict__.get("_addr_gen", 0)
        fp = m._flat_params
        quick = (fp.data_ptr() if fp is not None else 0, m.gradbuf().flat.data_ptr()) + tuple(self._extra_ptrs())
        if gen != getattr(self, "_addr_gen", None) or quick != getattr(self, "_quick_ptrs", None):
            if self._param_ptrs() != self._ptrs:
                raise RuntimeError("%s: a parameter or the gradient buffer moved after capture" % type(self).__name__)
            self._addr_gen, self._quick_ptrs = gen, quick

    def run(self, redraw=True):
        if self._param_ptrs() != self._ptrs:
            raise RuntimeError(
                "GraphedStep: a parameter or the gradient buffer moved after capture (model.to(), a new "
                "optimizer flattening the parameters, ...): the graph still points at the old storage. "
                "Create the optimizer before the GraphedStep, or capture again.")
        self._check_text_cache()
        if redraw:
            self.redraw()
        if self._cycle is not None:
            if self.optimizer is not None:
                self.optimizer.check_captured()
                self.optimizer.sync_hyperparameters()  # (a few float compares; a scheduler's new lr: one small copy)
            self.graph.replay()
            if self._cycle.advance(self.optimizer is not None) and self.optimizer is not None:
                self.optimizer._opt_called = True  # (torch's schedulers warn unless they have seen an optimizer step)
            return self.total
        self.graph.replay()
        return self.total


class SplitGraphedStep(GraphedStep):
    """The same captured step cut where the reference's loop holds the reins (train.py:64-72): THREE graphs over one
    memory pool -- `model(**batch)` | `criterion(outputs, batch)` | `loss.backward()` -- so that the unchanged caller's
    `optimizer.zero_grad()` between the second and the third lands where it always did (mesm_amd/autograph.py replays
    them from inside MESM.forward, Criterion.forward and ONE autograd node's backward: the structure of
    torch.cuda.make_graphed_callables, with this build's arena / draw / capacity machinery).  The activations the
    backward graph reads live in the pool until the next forward replay overwrites them: one forward in flight."""

    def __init__(self, *a, **kw):
        if kw.get("reducer") is not None:
            raise ValueError("SplitGraphedStep: gradient collectives ride in the one-graph step (GraphedStep)")
        if kw.get("micro_steps") is not None or kw.get("optimizer") is not None:
            raise ValueError("SplitGraphedStep: micro_steps / optimizer= belong to the one-graph step (GraphedStep): the "
                             "caller of the three-graph step owns zero_grad and the optimizer")
        super().__init__(*a, **kw)

    def _capture(self, side):
        if self._pull is not None:
            raise RuntimeError("SplitGraphedStep: MESM_STEP_PULL is a one-graph option")
        pool = torch.cuda.graph_pool_handle()
        self.g_fwd, self.g_crit, self.g_bwd = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        b = self.batch
        kw = dict(stream=side, pool=pool, capture_error_mode="thread_local")
        with torch.cuda.graph(self.g_fwd, **kw):
            self.counter.add_(1)
            out = self.model(**b, dataset_name=self.dataset_name, is_training=True, plan=self.plan)
        with torch.cuda.graph(self.g_crit, **kw):
            losses, total = self.crit(out, b, True)
        self.model.zero_grad(set_to_none=True)
        with torch.cuda.stream(side):
            self.seed = torch.ones_like(total)
        with torch.cuda.graph(self.g_bwd, **kw):
            total.backward(self.seed)
        gb = self.model.gradbuf()
        self.grad_params = [p for p in gb.params if p.grad is not None]
        self.out = map_tree(lambda k, t: t.detach() if torch.is_tensor(t) else t, out)
        self.total = total.detach()
        # the loss entries are elements of ONE vector (criterion.loss_entries): a replay hands out a copy of it, one launch
        pack = loss_pack(losses)
        self.loss_vec = pack.vec.detach() if pack is not None else None
        self.loss_index = {k: int(v._i) for k, v in losses.items()} if pack is not None else None
        self.losses = {k: v.detach() for k, v in losses.items()}

    def run(self, redraw=True):
        raise RuntimeError("SplitGraphedStep is replayed in three parts (forward_replay / criterion_replay / backward_replay)")

    def forward_replay(self):
        self._check_addresses()
        self._check_text_cache()
        self.g_fwd.replay()
        return self.out

    def criterion_replay(self):
        self.g_crit.replay()
        if self.loss_vec is not None:
            from .criterion import loss_entries
            losses = loss_entries(self.loss_vec.clone(), self.loss_index)  # (float() of all entries = one transfer)
        else:
            losses = {k: v.clone() for k, v in self.losses.items()}
        return losses, self.total

    def backward_replay(self, grad=None):
        if grad is not None:
            self.seed.copy_(grad)
        self.g_bwd.replay()


class EvalGraphedStep(GraphedStep):
    """The evaluation call of the reference (eval.py:63,102), forward only, captured in ONE graph:
    `model(**batch, is_training=False)` with the model in eval() mode (no dropout, no masked-LM branch, no backward) and,
    with a criterion, `criterion(outputs, batch, is_training=False)` behind it.  The arena, the index plans (the eval
    plan: no masked-word arrays), the capacities and the pair padding are GraphedStep's.  The one host draw of the
    forward -- the negative query index (sample_outclass_neg) -- is the caller's: `load_batch` keeps `_draws`, which the
    caller sets before every replay (autograph.py draws it exactly where the eager call would).

    Everything the replay wrote -- outputs, the loss vector, the total -- is packed inside the graph into ONE static byte
    buffer (`pack`), so that a caller takes its own copy of a replay with a single device copy (`replay_copy`)."""
    TRAIN = False
    DRAWN = ("p.neg_index",)

    def __init__(self, model, criterion, batch, dataset_name, warmup=1, caps=None, group_cap=None, neg_index=None):
        """criterion None: the forward alone.  neg_index: the draw of the first replay (None: drawn here)"""
        if model.training:
            raise ValueError("EvalGraphedStep: call model.eval() first (the step is captured in the model's mode)")
        self._targets = criterion is not None
        self._draws = (None if neg_index is None else neg_index, None)
        with torch.no_grad():
            super().__init__(model, criterion, batch, dataset_name, warmup=warmup, caps=caps, group_cap=group_cap)

    def _host_arrays(self, host, neg_index, masked_words, targets=True):
        if neg_index is None and getattr(self, "arena", None) is None:
            neg_index = self._draws[0]  # (the capture's own draw, handed in by the caller)
        return super()._host_arrays(host, neg_index, None, targets)

    def _step_body(self):
        b = self.batch
        out = self.model(**b, dataset_name=self.dataset_name, is_training=False, plan=self.plan)
        losses = total = None
        if self.crit is not None:
            losses, total = self.crit(out, b, False)
        return out, losses, total

    def _capture(self, side):
        with torch.cuda.graph(self.graph, stream=side, capture_error_mode="thread_local"):
            self.counter.add_(1)
            out, losses, total = self._step_body()
            self._pack_outputs(out, losses, total)

    def _pack_outputs(self, out, losses, total):
        """(captured) every output tensor, the loss vector and the total, byte-wise into one buffer; `layout` remembers
        where each one sits: [(path, dtype, shape, byte offset)] with path = key or (key, layer, subkey)"""
        items = []
        for k, v in out.items():
            if isinstance(v, list):
                for i, d in enumerate(v):
                    items += [((k, i, kk), vv) for kk, vv in d.items() if torch.is_tensor(vv)]
            elif torch.is_tensor(v):
                items.append((k, v))
        self.loss_index = None
        if losses is not None:
            pack = loss_pack(losses)
            if pack is not None:
                items.append((("_loss_vec",), pack.vec))
                self.loss_index = {k: int(v._i) for k, v in losses.items()}
            else:
                for k, v in losses.items():
                    items.append((("_loss", k), v.reshape(1)))
            items.append((("_total",), total.reshape(1)))
        items.sort(key=lambda kv: -kv[1].element_size())  # (largest element first: every piece stays aligned)
        self.layout, off = [], 0
        parts = []
        for path, t in items:
            t = t.detach().contiguous()
            nb = t.numel() * t.element_size()
            self.layout.append((path, t.dtype, tuple(t.shape), off, nb))
            parts.append(t.view(-1).view(torch.uint8))
            off += nb
        self.pack = torch.cat(parts)
        self.out_keys = list(out.keys())
        self.total_shape = tuple(total.shape) if total is not None else None

    def replay(self):
        """replay the captured call on the loaded batch and draws; -> a fresh copy of its pack (caller-owned memory)"""
        self._check_addresses()
        self._check_text_cache()
        self.graph.replay()
        return self.pack.clone()

    def unpack(self, buf):
        """views of a pack copy: (outputs in the eager call's key structure, losses {name: tensor} or None, total or None)"""
        got, losses, total, aux, vec = {}, {}, None, {}, None
        for path, dt, shape, off, nb in self.layout:
            t = buf[off:off + nb].view(dt).view(shape)
            if isinstance(path, str):
                got[path] = t
            elif path[0] == "_loss_vec":
                vec = t
            elif path[0] == "_loss":
                losses[path[1]] = t.reshape(())
            elif path[0] == "_total":
                total = t.view(self.total_shape)
            else:
                aux.setdefault(path[0], {}).setdefault(path[1], {})[path[2]] = t
        for k, layers in aux.items():
            got[k] = [layers[i] for i in sorted(layers)]
        out = {k: got[k] for k in self.out_keys if k in got}
        if vec is not None:
            from .criterion import loss_entries
            losses = loss_entries(vec, self.loss_index)
        return out, (losses if self.crit is not None else None), total

    def run(self, redraw=True):
        raise RuntimeError("EvalGraphedStep is replayed with replay() / unpack()")


class GraphCache:
    """Captured steps by bucket key, for StepCache and both paths of autograph.AutoGraph: key -> [steps] (a bucket can need
    more than one graph: other plan switches, capacities the first one lacks), at most `max_graphs` GRAPHS in all, the least
    recently used key evicted first (a hit refreshes it).  `captures` / `replays` count for the owner; `seen` (the bucket
    shapes visited) and `bad` (keys whose capture failed) are autograph.AutoGraph's bookkeeping."""

    def __init__(self, max_graphs=16):
        self.steps = OrderedDict()
        self.max_graphs = max_graphs
        self.seen = set()
        self.bad = set()
        self.captures = 0
        self.replays = 0

    def find(self, key, load):
        """the first step of bucket `key` that load(step) takes (ValueError: the batch does not fit it), or None"""
        for s in self.steps.get(key, ()):
            try:
                load(s)
            except ValueError:
                continue
            self.steps.move_to_end(key)
            return s
        return None

    def add(self, key, capture):
        """evict until one more graph fits the budget, then capture() -> a new step of bucket `key`"""
        while self.steps and sum(len(v) for v in self.steps.values()) >= self.max_graphs:
            self.steps.popitem(last=False)
        step = capture()
        self.steps.setdefault(key, []).append(step)
        self.captures += 1
        return step

    def first_visit(self, key, shape=None):
        """count a visit of bucket `key` (visits are counted per `shape`, default the key): True on the first one of a key
        without graphs -- it runs eagerly, the next one captures"""
        shape = key if shape is None else shape
        first = key not in self.steps and shape not in self.seen
        self.seen.add(shape)
        return first

    def drop(self):
        """forget the graphs and the visits that led to them (they were captured with another criterion object)"""
        if self.steps:
            self.steps.clear()
            self.seen.clear()


class StepCache(GraphCache):
    """One captured graph per batch-shape bucket: `run(batch)` replays a graph whose shape key
    (N, Lv, Lw, feature dims) and capture-time capacities (largest video group, GT-clip count, group video
    length, target windows) fit the batch, capturing a new one when none does.  `pad=(Lv_cap, Lw_cap)` first
    pads every batch to fixed clip / word extents (batching.shape_batch), so that the key is the number of pairs alone:
    real loaders emit a different (N, Lv, Lw, grouping) almost every batch -- items are videos with all their queries,
    dataset/base.py:164-207 -- and only a handful of distinct N.  `captures` counts the graphs built."""

    def __init__(self, model, criterion, dataset_name, reducer=None, max_graphs=16, pad=None, pairs=None,
                 group_caps=None, micro_steps=None, optimizer=None, grad_clip=0.0):
        """pairs: also pad the PAIR axis up to the next multiple of `pairs` (batching.pad_pairs: dummy pairs behind
        the real ones, the real count a device scalar of the captured step) -- the reference's loaders emit a different
        number of pairs almost every batch (an item is a video with all its queries, dataset/base.py:116-162), and
        with pairs=8 a QVHighlights epoch of 12-group batches replays from a handful of graphs.
        group_caps: ascending group-size buckets, e.g. (5, 9): a batch is served by a graph captured with room for
        video groups of up to the smallest bucket that holds its largest group (9 = the QVHighlights maximum), so that
        (pair bucket, group bucket) alone decide which graph a batch replays -- groups cost SS-MESM key slots
        (group size x clips per pair), which is why there is more than one bucket.
        micro_steps / optimizer / grad_clip: GraphedStep's, for every graph of the cache; the graphs share the model's
        cycle state, so the micro-batches of one cycle may fall into different buckets."""
        super().__init__(max_graphs)
        self.model, self.crit, self.dataset_name = model, criterion, dataset_name
        self.reducer = reducer
        self._micro = dict(micro_steps=micro_steps, optimizer=optimizer, grad_clip=grad_clip)
        self._cycle = None
        if micro_steps is not None or optimizer is not None:
            GraphedStep._check_micro_args(self, model, reducer, micro_steps, optimizer)
            self._cycle = model.gradbuf().cycle_state(next(model.parameters()).device)
            self._cycle.set_k(micro_steps)
        self.pad = pad
        self.pairs = pairs
        self.group_caps = tuple(sorted(group_caps)) if group_caps else None

    def run(self, batch, redraw=True, draws=None):
        """draws: (neg_index, masked_words) to replay with (GraphedStep.set_draws: tests, reproducing a recorded step)
        instead of drawing"""
        if draws is not None:
            redraw = False
        batch = shape_batch(batch, self.pad, self.pairs)
        k = bucket_key(batch, self.group_caps)
        gs = self.find(k, lambda s: s.load_batch(batch, redraw=redraw))
        if gs is not None:
            self.replays += 1
            if draws is not None:
                gs.set_draws(*draws)
            return gs.run(redraw=False), gs
        dev = next(self.model.parameters()).device
        gs = self.add(k, lambda: GraphedStep(self.model, self.crit, capture_batch(batch, dev), self.dataset_name, warmup=1,
                                             reducer=self.reducer, caps="auto", group_cap=k[2] if self.group_caps else None,
                                             **self._micro))
        if draws is not None:
            gs.set_draws(*draws)
        return gs.run(redraw=redraw), gs

    TRAIN = True
    micro_steps = GraphedStep.micro_steps
    update_due = GraphedStep.update_due
    updates = GraphedStep.updates
    set_micro_steps = GraphedStep.set_micro_steps
    reset_cycle = GraphedStep.reset_cycle

    def pipeline(self, keep_raw=True):
        """the host half of `run` as a picklable object for loader workers (loader.HostPipeline).  keep_raw=False once
        every bucket of the stream has its graph: the raw batch (needed only to capture) then does not travel."""
        from .hostplan import HostSpec
        from .loader import HostPipeline
        return HostPipeline(HostSpec.from_model(self.model, self.crit, self.dataset_name), pad=self.pad, pairs=self.pairs,
                            group_caps=self.group_caps, keep_raw=keep_raw)

    def run_prepared(self, prep):
        """`run` for a batch prepared by a loader worker (loader.HostPipeline.prepare): the graph of its bucket key takes
        the arrays as they are (the two host draws are made here); a bucket without a graph yet goes through `run` on
        the raw batch the worker kept alongside (prep["raw"]), which captures it."""
        gs = self.find(prep["key"], lambda s: s.load_prepared(prep))
        if gs is not None:
            self.replays += 1
            return gs.run(redraw=False), gs
        if prep.get("raw") is None:
            raise ValueError("StepCache.run_prepared: no graph for bucket %r and the prepared batch carries no raw batch" % (prep["key"],))
        return self.run(prep["raw"], redraw=True)
