"""Graph replay behind the UNCHANGED caller (reference train.py:64-72):

    outputs = model(**batch, dataset_name=..., is_training=True)
    loss_dict, loss = criterion(outputs, batch, is_training=True)
    optimizer.zero_grad()
    loss.backward()
    clip_grad_norm_(model.parameters(), ...); optimizer.step()

The eager path issues ~260 launches from Python and is host-bound (17 ms per step where the device needs 3.5).  An
`AutoGraph` hangs off every `MESM` and turns that same call sequence into three HIP-graph replays
(graphed.SplitGraphedStep: forward | criterion | backward over one memory pool) once a batch shape has been seen:

  * first visit of a shape bucket: eager, exactly as before (it is also the step the criterion introduces itself in:
    `Criterion.forward` finds the model on the outputs it is handed);
  * second visit: the bucket is captured (warm-up step + three captures; the caller's gradients are put back as they
    were) and replayed; from then on `model(...)` = host plans + one arena upload + forward replay,
    `criterion(...)` = criterion replay, `loss.backward()` = ONE autograd node whose backward replays the third graph
    and leaves `param.grad` aliasing the flat gradient buffer like the eager backward does.  `optimizer.zero_grad()`
    in between, `clip_grad_norm_`, any `torch.optim` optimizer: unchanged.  Gradients ACCUMULATE when `param.grad` is
    not None at backward time (the caller skipped zero_grad), like autograd's.

What a replayed step cannot do, and says so instead of computing something else: the activations the backward reads are
static memory that the next forward overwrites, so ONE forward may be in flight -- a backward (or criterion call) that
belongs to an older forward raises; the outputs carry no autograd history of their own (they are consumed by this
build's criterion; anything else that wants gradients through them needs the eager path).  `MESM_AUTOGRAPH=0`, or
`model.autograph(False)`, keeps every step eager.

Evaluation calls (eval.py:63,102: `model(**batch, is_training=False)` under no_grad with the model in eval() mode, then
`criterion(outputs, batch, is_training=False)`) stay eager unless asked: `model.autograph(eval=True)` or
MESM_AUTOGRAPH_EVAL=1 replays them from forward-only graphs (graphed.EvalGraphedStep: the forward and, once the criterion
is known and the batch carries its targets, the criterion in the same graph).  Same rules as training -- eager first
visit, capture on the second, pad / pairs buckets -- with a cache of their own (their own budget: evaluation never evicts
a training graph, nor the other way round).  The negative-query draw is made where the eager call makes it, from the
same global RNG stream.  The outputs are the caller's: one device copy out of graph memory, cut to the real pairs and the
caller's clip / word extents; `criterion(outputs, batch, is_training=False)` with that batch returns the losses of the
same replay, with any other batch it runs eagerly on those copies.

Buckets: key = (dataset, train/eval mode, pairs, clip / word extents, feature dims, group-size bucket, batch keys).
The reference's loaders emit another (pairs, Lv, Lw) almost every batch; `model.autograph(pad=(max_v_l, max_words_l),
pairs=8)` pads every batch like graphed.StepCache does (clips / words to fixed extents, the pair axis to a multiple of
`pairs` with the real count as a device scalar), so that an epoch replays from a handful of graphs.
"""
import os
import warnings
import weakref

import torch

from . import kernels as kn
from .batching import feature_tag, group_bucket, shape_batch


class AutoOutputs(dict):
    """the dict MESM.forward returns, remembering which forward made it (a plain dict to every reader)"""
    _mesm_model = None   # weakref to the model (eager and replayed outputs)
    _auto_step = None    # the SplitGraphedStep whose forward graph wrote these tensors (replayed outputs only)
    _auto_gen = -1
    _auto_batch = None
    _mesm_side = None    # the stream an eager forward ran on when that was not the caller's (eager outputs only)
    _eval_losses = None  # (losses, total) captured with a replayed evaluation forward (replayed eval outputs only)


class _Backward(torch.autograd.Function):
    """loss = f(token): the ONE node of a replayed step; its backward replays the third graph"""

    @staticmethod
    def forward(ctx, token, total, auto, step, gen):
        ctx.auto, ctx.step, ctx.gen = auto, step, gen
        return total.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.auto.backward(ctx.step, ctx.gen, g)
        return None, None, None, None, None


_NP = {torch.float32: "float32", torch.float64: "float64", torch.int64: "int64", torch.int32: "int32",
       torch.bool: "bool", torch.uint8: "uint8", torch.int16: "int16", torch.float16: "float16", torch.int8: "int8"}


class _Fetch:
    """Everything small of a DEVICE batch (prepare_batch_input has moved it there, dataset/base.py:358-384) back on the host
    in ONE transfer: the index plans and the flattened targets are host arithmetic on masks, labels and target windows (a few
    KB), and one `.cpu()` per tensor is one stream synchronisation each -- 77 per C3a batch, 1.2 ms.  The tensors are packed
    by one concatenation kernel (largest element size first, so every piece stays aligned), copied into a pinned buffer and
    cut into numpy views.  The per-pair target lists travel as one tensor per entry; the word-validity mask of pre-extracted
    word features (2 MB of features otherwise) is formed on the device with hostplan.HostSpec.words_mask's arithmetic."""

    def __init__(self):
        self.pinned = None

    def __call__(self, batch, spec, big):
        import numpy as np
        items, lists = [], {}
        for k, v in batch.items():
            if torch.is_tensor(v):
                if v.is_cuda and v.dtype in _NP and v.numel() * v.element_size() <= big:
                    items.append((k, v))
            elif isinstance(v, list) and v and isinstance(v[0], dict):
                for kk in v[0]:
                    ts = [d[kk] for d in v]
                    if all(torch.is_tensor(t) and t.is_cuda for t in ts):
                        lists[(k, kk)] = [int(t.shape[0]) for t in ts]
                        items.append(((k, kk), torch.cat(ts)))
        w = batch["words_id"]
        if w.dim() == 3 and w.is_cuda:
            a = w
            if spec.normalize_txt:
                a = a / a.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-5)
            items.append(("_words_mask", a.sum(-1) != 0))
        items.sort(key=lambda kv: -kv[1].element_size())
        flat = torch.cat([t.contiguous().view(-1).view(torch.uint8) for _, t in items])
        n = flat.numel()
        if self.pinned is None or self.pinned.numel() < n:
            self.pinned = torch.empty(max(2 * n, 1 << 16), dtype=torch.uint8, pin_memory=True)
        self.pinned[:n].copy_(flat, non_blocking=True)
        torch.cuda.current_stream(flat.device).synchronize()
        raw = self.pinned.numpy()[:n].copy()  # (the pinned buffer is reused by the next batch)
        host, off = {}, 0
        for key, t in items:
            nb = t.numel() * t.element_size()
            arr = raw[off:off + nb].view(_NP[t.dtype]).reshape(tuple(t.shape))
            off += nb
            host[key] = torch.from_numpy(arr)
        out = {}
        for k, v in batch.items():
            if torch.is_tensor(v):
                out[k] = host.get(k, v)
            elif isinstance(v, list) and v and isinstance(v[0], dict) and all((k, kk) in lists for kk in v[0]):
                parts = {kk: host[(k, kk)].split(lists[(k, kk)]) for kk in v[0]}
                out[k] = [{kk: parts[kk][i] for kk in v[0]} for i in range(len(v))]
        if "_words_mask" in host:
            out["_words_mask"] = host["_words_mask"]
        return out


def _enabled_default():
    return os.environ.get("MESM_AUTOGRAPH", "1") != "0"


def _eval_default():
    return os.environ.get("MESM_AUTOGRAPH_EVAL", "0") == "1"


# evaluation outputs with a clip axis / a word axis (+ leading sentence slot) at dim 1: cut back to the caller's extents
_EVAL_CLIP_OUT = ("saliency_scores", "neg_saliency_scores", "projed_video_feat", "enhanced_video_feat")
_EVAL_WORD_OUT = {"projed_words_feat": 0, "expanded_words_feat": 1, "expanded_words_mask": 1, "words_mask": 0}


GROUP_CAPS = (1, 2, 3, 5, 9, 16, 32, 64)  # largest-video-group buckets (9 = the QVHighlights maximum, base.py:116-162)


class AutoGraph:
    def __init__(self, model):
        from .graphed import GraphCache
        self.model = weakref.ref(model)
        self.enabled = _enabled_default()
        self.crit = None
        self.train_graphs = GraphCache(int(os.environ.get("MESM_AUTOGRAPH_MAX", "16")))  # SplitGraphedStep
        self.pad = None
        self.pairs = None
        self.gen = 0          # forwards of this model (eager ones included): one may be in flight
        self.busy = False     # inside a capture: the model's forward is being called by the step itself
        self.token = None
        self.eager = 0        # first visits of a training bucket (run eagerly)
        self.fetch = _Fetch()
        self.spec, self._spec_key = None, None  # hostplan.HostSpec of (dataset, criterion object)
        self.host_side = 0    # forwards served from the collate's host copies (batch["_host"]) instead of a fetch
        # evaluation calls (opt-in): their own graphs, budget and counters
        self.eval_enabled = _eval_default()
        self.eval_graphs = GraphCache(int(os.environ.get("MESM_AUTOGRAPH_EVAL_MAX", "16")))  # EvalGraphedStep
        self.eval_eager = 0   # evaluation calls that ran eagerly
        self.eval_neg = None  # the draw of an eval call that ends up eager after all (it has been made already)

    captures = property(lambda self: self.train_graphs.captures)
    replays = property(lambda self: self.train_graphs.replays)
    bad = property(lambda self: self.train_graphs.bad)
    eval_captures = property(lambda self: self.eval_graphs.captures)
    eval_replays = property(lambda self: self.eval_graphs.replays)

    # ------------------------------------------------------------------ configuration
    def configure(self, enabled=None, pad=None, pairs=None, max_graphs=None, eval=None):
        if enabled is not None:
            self.enabled = bool(enabled)
        if eval is not None:
            self.eval_enabled = bool(eval)
        if pad is not None:
            self.pad = tuple(pad)
        if pairs is not None:
            self.pairs = int(pairs)
        if max_graphs is not None:
            self.train_graphs.max_graphs = int(max_graphs)
        return self

    def note_criterion(self, crit):
        if self.crit is None or self.crit() is not crit:
            self.crit = weakref.ref(crit)
            # graphs captured with another criterion object: its weights / losses are baked in
            self.train_graphs.drop()
            self.eval_graphs.drop()
            self.spec = self._spec_key = None

    # ------------------------------------------------------------------ forward
    @staticmethod
    def _with_host_side(batch, spec):
        """the batch with its small tensors replaced by the host copies the collate kept (batching.attach_host_side) -> a dict
        that serves both as the shaped batch (big device tensors) and as the host half (everything else), or None when
        `_host` is absent / does not mirror the batch"""
        hs = batch.get("_host")
        if not isinstance(hs, dict):
            return None
        work = {}
        for k, v in batch.items():
            if k == "_host":
                continue
            if torch.is_tensor(v) and v.is_cuda and k in hs:
                h = hs[k]
                if not torch.is_tensor(h) or h.is_cuda or tuple(h.shape) != tuple(v.shape) or h.dtype != v.dtype:
                    return None
                work[k] = h
            elif isinstance(v, list) and v and isinstance(v[0], dict) and k in hs:
                if len(hs[k]) != len(v):
                    return None
                work[k] = hs[k]
            elif torch.is_tensor(v) and v.is_cuda and v.numel() * v.element_size() <= (1 << 20):
                return None  # a small device tensor the collate did not keep: fetch instead
            else:
                work[k] = v
        w = batch["words_id"]
        if w.dim() == 3:
            m = hs.get("_words_mask_norm" if spec.normalize_txt else "_words_mask_raw")
            if m is None or tuple(m.shape) != tuple(w.shape[:2]):
                return None
            work["_words_mask"] = m
        return work

    def _prepare(self, model, batch, dataset_name, crit, train):
        """what both paths do before they look for a graph -> (shaped batch, its host half or None, bucket key, group bucket),
        or None: this call runs eagerly (a batch beyond `pad`, or anything the host half cannot handle).  The shaped batch is
        padded like StepCache pads (device tensors stay on the device).  The host half comes from the collate's host copies
        (counted in `host_side` for training) or from one fetch; the training path makes none before a criterion is known."""
        try:
            work = None
            fetch = crit is not None or not train
            if fetch:
                if self._spec_key != (dataset_name, id(crit)):
                    from .hostplan import HostSpec
                    self.spec, self._spec_key = HostSpec.from_model(model, crit, dataset_name), (dataset_name, id(crit))
                work = self._with_host_side(batch, self.spec)
            if work is not None:
                # the collate kept the host copies: no transfer back, no synchronisation in front of the forward launch
                if train:
                    self.host_side += 1
                shaped = host = shape_batch(work, self.pad, self.pairs)
            else:
                shaped = shape_batch({k: v for k, v in batch.items() if k != "_host"}, self.pad, self.pairs)
                host = None
                if fetch:
                    from .graphed import GraphedStep
                    host = self.fetch(shaped, self.spec, GraphedStep.BIG)
            key, gcap = self._key(model, shaped, dataset_name, None if host is None else host["num_clips"])
        except Exception:
            return None
        return shaped, host, key, gcap

    @staticmethod
    def _key(model, batch, dataset_name, num_clips=None):
        n = batch["video_mask"].shape[0]
        gcap = group_bucket(batch["num_clips"] if num_clips is None else num_clips, GROUP_CAPS)
        sig = tuple(sorted(k for k, v in batch.items() if not k.startswith("_")))
        return (dataset_name, bool(model.training), n, tuple(batch["video_feat"].shape[1:]),
                tuple(batch["words_id"].shape[1:]), gcap, "_n_real" in batch, sig) + feature_tag(batch), gcap

    def eligible(self, model, batch, kwargs):
        return (self.enabled and not self.busy and kwargs.get("is_training") is True and kwargs.get("plan") is None
                and torch.is_grad_enabled() and batch["video_feat"].is_cuda
                and kwargs.get("neg_index") is None and kwargs.get("masked_words") is None
                and not torch.cuda.is_current_stream_capturing())

    def eligible_eval(self, model, batch, kwargs):
        return (self.enabled and self.eval_enabled and not self.busy and kwargs.get("is_training") is False
                and not torch.is_grad_enabled() and not model.training and kwargs.get("plan") is None
                and kwargs.get("neg_index") is None and kwargs.get("masked_words") is None
                and batch["video_feat"].is_cuda and not torch.cuda.is_current_stream_capturing())

    def eager_stream(self, dev):
        """the stream an EAGER grad-enabled forward of a caller on the default stream runs on (None: where the caller is)"""
        if not self.enabled or self.busy or not torch.is_grad_enabled() or torch.cuda.is_current_stream_capturing():
            return None
        if torch.cuda.current_stream(dev) != torch.cuda.default_stream(dev):
            return None
        from .graphed import capture_stream
        return capture_stream(dev)

    def forward(self, batch, dataset_name):
        """-> AutoOutputs of a replayed forward, or None: run this forward eagerly"""
        model = self.model()
        self.gen += 1
        if model.gradbuf().on_ready is not None:
            # a ddp.GradReducer is hooked into the gradient buffer: its collectives belong in the one-graph step that was
            # built WITH the reducer (GraphedStep / StepCache(reducer=...)), not in a capture made behind its back
            return None
        crit = self.crit() if self.crit is not None else None
        got = self._prepare(model, batch, dataset_name, crit, train=True)
        if got is None:
            return None
        shaped, host, key, gcap = got
        cache = self.train_graphs
        if key in cache.bad:
            return None
        # (the visit counts without a criterion as well: the first step is the one the criterion introduces itself in)
        if cache.first_visit(key) or crit is None:
            self.eager += 1
            return None
        step = cache.find(key, lambda s: s.load_batch(shaped, redraw=True, host=host, defer_targets=True))
        if step is None:
            step = self._capture_train(key, gcap, shaped, dataset_name, crit)
            if step is None:
                return None
        out = step.forward_replay()
        if step._pending_targets is not None:
            try:
                step.finish_targets()  # (the criterion's arrays, while the forward graph runs)
            except ValueError:
                return None  # targets beyond the captured capacities: this step runs eagerly
        cache.replays += 1
        n = batch["video_feat"].shape[0]
        if shaped["video_mask"].shape[0] != n:  # a pair-padded replay: the caller's pairs (views)
            from .graphed import map_tree
            out = map_tree(lambda k, t: t[:n] if torch.is_tensor(t) and t.dim() >= 1 else t, out)
        res = AutoOutputs(out)
        res._mesm_model = self.model
        res._auto_step, res._auto_gen, res._auto_batch = step, self.gen, batch
        return res

    # ------------------------------------------------------------------ evaluation forward
    _TARGETS = ("norm_span", "norm_moment", "video_mask")

    def forward_eval(self, batch, dataset_name):
        """-> AutoOutputs of a replayed evaluation call, or None: run it eagerly (with `eval_neg` when the draw is made)"""
        from . import draws
        self.eval_neg = None
        model = self.model()
        crit = self.crit() if self.crit is not None else None
        with_crit = crit is not None and all(k in batch for k in self._TARGETS) \
            and ("saliency_label" in batch or "clip_mask" in batch)
        got = self._prepare(model, batch, dataset_name, crit, train=False)
        if got is None:
            self.eval_eager += 1
            return None
        shaped, host, seen_key, gcap = got
        key = seen_key + (with_crit,)
        cache = self.eval_graphs
        # (visits are counted per shape: the first call of an epoch may come before the criterion introduced itself)
        first = cache.first_visit(key, seen_key)
        if key in cache.bad or first:
            self.eval_eager += 1
            return None
        # the eager call's one host draw, here: same stream, same place in it (the real groups; padding pairs -> 0)
        neg = draws.neg_index([int(g) for g in host["num_clips"].tolist()], shaped.get("_n_real"))
        n = batch["video_feat"].shape[0]
        self.eval_neg = neg[:n]

        def load(s):
            s._draws = (neg, None)
            s.load_batch(shaped, redraw=False, host=host)
        step = cache.find(key, load)
        if step is None:
            from .graphed import EvalGraphedStep, capture_batch

            def capture():
                s = EvalGraphedStep(model, crit if with_crit else None, capture_batch(shaped, shaped["video_feat"].device),
                                    dataset_name, warmup=1, caps="auto", group_cap=gcap if gcap > 1 else None, neg_index=neg)
                self._check_eval_axes(model, s, shaped)
                return s
            step = self._capture(cache, key, capture, "eval capture")
            if step is None:
                self.eval_eager += 1
                return None
        buf = step.replay()
        out, losses, total = step.unpack(buf)
        self.eval_neg = None
        cache.replays += 1
        res = AutoOutputs(self._eval_extents(model, out, batch, n))
        res._mesm_model = self.model
        res._auto_batch = batch
        if losses is not None:
            res._eval_losses = (losses, total)
        return res

    @staticmethod
    def _extents(model, batch):
        """(clips, words) of the forward's outputs for `batch` (token ids are cut to max_words_l by the CLIP encoder)"""
        W = batch["words_id"]
        Lw = W.shape[1]
        if W.dim() == 2:
            from .text_encoder import CLIPTextEncoder
            if isinstance(model.text_encoder, CLIPTextEncoder):
                Lw = min(Lw, model.max_words_l)
        return batch["video_feat"].shape[1], Lw

    def _check_eval_axes(self, model, step, shaped):
        """a graph of padded clip / word extents (pad=...) serves callers of smaller ones, so it may only hand out outputs
        whose clip / word axis the cut knows (_EVAL_CLIP_OUT / _EVAL_WORD_OUT): any other output with such an extent at
        dim 1 -- a new output of the model -- refuses the capture (the shape stays eager) instead of coming back padded"""
        if self.pad is None:
            return
        Lv_p, Lw_p = AutoGraph._extents(model, shaped)
        padded = {Lv_p} | {Lw_p + c for c in set(_EVAL_WORD_OUT.values())}
        for path, _, shape, _, _ in step.layout:
            k = path if isinstance(path, str) else (path[2] if len(path) == 3 else None)
            if k is None or len(shape) < 2 or k in _EVAL_CLIP_OUT or k in _EVAL_WORD_OUT:
                continue
            if shape[1] in padded:
                raise ValueError("output %r %s has a padded clip / word extent at dim 1 that the eval cut does not know"
                                 % (k, shape))

    @staticmethod
    def _eval_extents(model, out, batch, n):
        """outputs of a padded replay with the eager call's shapes: the real pairs, the caller's clips and words (views)"""
        from .graphed import map_tree
        Lv, Lw = AutoGraph._extents(model, batch)

        def cut(k, t):
            if not torch.is_tensor(t) or t.dim() < 1:
                return t
            t = t[:n]
            if t.dim() >= 2:
                if k in _EVAL_CLIP_OUT:
                    t = t[:, :Lv]
                elif k in _EVAL_WORD_OUT:
                    t = t[:, :Lw + _EVAL_WORD_OUT[k]]
            return t
        return map_tree(cut, out)

    def eval_criterion(self, crit, outputs, targets, is_training):
        """the losses captured with a replayed evaluation forward, or None (the caller runs the eager criterion)"""
        if is_training or self.crit is None or self.crit() is not crit or outputs._eval_losses is None:
            return None
        b = outputs._auto_batch
        if targets is not b and any(targets.get(k) is not b.get(k) for k in b):
            return None
        losses, total = outputs._eval_losses
        return dict(losses), total

    def _capture(self, cache, key, capture, what="capture"):
        """cache.add(key, capture) with the model's forward reserved for the capture; a bucket whose capture fails stays
        eager (said once) -> the new step or None"""
        self.busy = True
        try:
            return cache.add(key, capture)
        except Exception as e:  # a shape this build cannot capture: stay eager for it, say so once
            cache.bad.add(key)
            warnings.warn("mesm_amd.autograph: %s failed for %r (%s: %s); this shape stays eager" % (what, key, type(e).__name__, e))
            return None
        finally:
            self.busy = False

    def _capture_train(self, key, gcap, batch, dataset_name, crit):
        from .graphed import SplitGraphedStep, capture_batch
        model = self.model()
        gb = model.gradbuf()
        # the warm-up and capture steps run real backward passes: the caller's gradients are put back afterwards
        had = [p.grad is not None for p in gb.params]
        saved = gb.flat.clone() if (gb.flat is not None and any(had)) else None
        try:
            return self._capture(self.train_graphs, key, lambda: SplitGraphedStep(
                model, crit, capture_batch(batch, batch["video_feat"].device), dataset_name, warmup=1, caps="auto",
                group_cap=gcap if gcap > 1 else None))
        finally:
            if saved is not None:
                gb.flat.copy_(saved)
            for p, h in zip(gb.params, had):
                p.grad = p._mesm_gview if h else None

    # ------------------------------------------------------------------ criterion / backward
    def _check(self, step, gen, what):
        if gen != self.gen:
            raise RuntimeError(
                "mesm_amd.autograph: %s of a forward that is no longer the latest one of this model -- a replayed step keeps "
                "its activations in static graph memory, so only ONE forward may be in flight (forward -> criterion -> "
                "backward).  Set MESM_AUTOGRAPH=0 (or model.autograph(False)) for patterns that interleave forwards." % what)

    def criterion(self, crit, outputs, targets, is_training):
        step = outputs._auto_step
        self._check(step, outputs._auto_gen, "criterion call on the outputs")
        if self.crit is None or self.crit() is not crit:
            raise RuntimeError("mesm_amd.autograph: these outputs belong to a step captured with another criterion object; "
                               "call model.autograph(False) to mix criteria")
        if not is_training:
            raise RuntimeError("mesm_amd.autograph: criterion(..., is_training=False) on the outputs of a training forward")
        b = outputs._auto_batch
        if targets is not b and any(targets.get(k) is not b.get(k) for k in ("video_mask", "saliency_label", "norm_span", "words_label")):
            raise RuntimeError("mesm_amd.autograph: the criterion's targets are not the batch the forward was called with "
                               "(a replayed step reads its targets when the forward starts)")
        losses, total = step.criterion_replay()
        if self.token is None or self.token.device != total.device:
            self.token = torch.zeros((), device=total.device, requires_grad=True)
        return losses, _Backward.apply(self.token, total, self, step, outputs._auto_gen)

    def backward(self, step, gen, g):
        self._check(step, gen, "backward")
        model = self.model()
        gb = model.gradbuf()
        prev = gb.flat.clone() if any(p.grad is not None for p in gb.params) else None
        step.backward_replay(g)
        if prev is not None:
            gb.flat.add_(prev)  # the captured backward starts from a cleared buffer: accumulate like autograd does
        for p in step.grad_params:
            if p.grad is None:
                p.grad = p._mesm_gview
