"""Flat fp32 gradient buffer shared by every trainable parameter of a model.

The kernels accumulate weight / bias / LayerNorm gradients straight into views of ONE
contiguous buffer (dW GEMMs with split-K atomics, LayerNorm dgamma/dbeta atomics), and
``param.grad`` is made to alias that view.  This keeps ``loss.backward()`` /
``optimizer.step()`` / ``clip_grad_norm_`` of the reference's train loop (train.py:68-72)
working unchanged while giving data-parallel training a single buffer to all-reduce
(ddp.py) instead of 262 tensors.

Zeroing protocol (matches ``optimizer.zero_grad()`` with set_to_none=True or False being
called anywhere between two backward passes, train.py:68): ``begin_step()`` is called by
the model's training forward; the first gradient written in the following backward checks
the parameters: all ``.grad is None`` -> one memset of the flat buffer; otherwise the
existing contents are kept (gradient accumulation) and only still-None views are zeroed.
Parameters that no kernel touches keep ``.grad = None`` exactly like under autograd.
"""
import torch


def _zero(t):
    """memset of a gradient buffer: on the GPU through mesm_fill_ranges (write-through stores: the 55 MB do not sit dirty
    in L2 until the end of the launch), elsewhere -- or for an odd size -- torch's fill"""
    if t.is_cuda and t.is_contiguous() and t.data_ptr() % 16 == 0 and (t.numel() * t.element_size()) % 16 == 0 and t.numel() > 0:
        from . import kernels as kn  # (late: kernels imports this module)
        kn.fill_zero(t)
    else:
        t.zero_()


class Pack:
    """Several parameters laid out back to back in the flat buffers, seen as ONE matrix / vector: e.g. the
    decoder's sa_qcontent / sa_kcontent / sa_v weights as a (3d, d) matrix, so that the three projections of the
    same input are one GEMM forward, one dX GEMM and one dW GEMM backward (and autograd has no gradient fan-in to
    add up).  `weight()` / `grad()` are views of the flat parameter / gradient buffers; a Pack quacks like a
    parameter for ops.grad_target (it acquires every member)."""

    def __init__(self, gb, members, shape):
        self.gb, self.members, self.shape = gb, members, shape
        self.offset = gb.offsets[next(i for i, q in enumerate(gb.params) if q is members[0])]
        self.numel = sum(m.numel() for m in members)
        self._w = None

    @property
    def flat(self):
        return self.gb.flat

    def weight(self, flat_params):
        """view of the flat PARAMETER buffer (model.flat_params()); carries the hooks grad_target looks for"""
        if self._w is None or self._w.data_ptr() != flat_params.data_ptr() + 4 * self.offset:
            w = flat_params[self.offset:self.offset + self.numel].view(self.shape)
            w._mesm_gb = self
            self._w = w
        return self._w

    def acquire(self, _w):
        for m in self.members:
            self.gb.acquire(m)
        return self.gb.flat[self.offset:self.offset + self.numel].view(self.shape)


class CycleState:
    """Where a model stands in a cycle of micro-batched graph replays (graphed.GraphedStep(micro_steps=k)): four int32 words
    of DEVICE memory, {count, k, phase, due} (include/mesm_gfx950.h, mesm_micro_begin), that every micro-stepped graph of
    the model shares -- the micro-batches of one cycle may replay different buckets' graphs -- plus what goes with them:
    `seed`, the 1 / k the captured backward is seeded with (a tensor, so that k changes without a new capture),
    and the host's own count of the replays (`pos`, `due`, `updates`), which needs no read-back.  On the device the first
    node of each graph is the only writer of the words; the host writes k and count between cycles only."""
    COUNT, K, PHASE, DUE = range(4)

    def __init__(self, device):
        self.words = torch.zeros(4, dtype=torch.int32, device=device)
        self.seed = torch.ones(1, dtype=torch.float32, device=device)
        self.k = 1
        self.words[self.K:self.K + 1].fill_(1)
        self.pos = 0          # replays done in the current cycle
        self.due = False      # the last replay was the k-th of its cycle
        self.updates = 0      # cycles completed by graphs that carry the optimizer tail
        self.covered = None   # per parameter: some micro-stepped graph of this model writes its gradient

    @property
    def phase_word(self):
        return self.words[self.PHASE:self.PHASE + 1]

    @property
    def due_word(self):
        return self.words[self.DUE:self.DUE + 1]

    def set_k(self, k):
        k = int(k)
        if k < 1:
            raise ValueError("micro_steps must be >= 1, got %d" % k)
        if k == self.k:
            return
        if self.pos != 0:
            raise RuntimeError("micro_steps changes at a cycle boundary only: %d of %d micro-steps of this cycle are "
                               "done (reset_cycle() drops them)" % (self.pos, self.k))
        self.k = k
        self.words[self.K:self.K + 1].fill_(k)
        self.seed.fill_(1.0 / k)

    def reset(self):
        """drop an unfinished cycle: the next replay is a first one (it clears the gradient buffer)"""
        self.words[self.COUNT:self.COUNT + 1].zero_()
        self.pos, self.due = 0, False

    def advance(self, with_update):
        """the host's mirror of mesm_micro_begin, after a replay has been launched"""
        self.pos += 1
        self.due = self.pos == self.k
        if self.due:
            self.pos = 0
            if with_update:
                self.updates += 1
        return self.due


class GradBuffer:
    def __init__(self, named_params, packs=None):
        """packs: {key: [parameter names]} -- members are placed back to back (in the given order) in the
        flat layout; every member's numel must be a multiple of 4.  The ORDER OF `params` (optimizer state
        indices, checkpoints) is unaffected: only `offsets` are permuted."""
        self.names = [n for n, _ in named_params]
        self.params = [p for _, p in named_params]
        by_name = dict(named_params)
        first_of, member_of = {}, set()
        for key, names in (packs or {}).items():
            assert all(by_name[n].numel() % 4 == 0 for n in names), key
            first_of[names[0]] = names
            member_of.update(names)
        off_of = {}
        off = 0
        for n, p in named_params:
            if n in off_of:
                continue
            for m in first_of.get(n, [n] if n not in member_of else []):
                off_of[m] = off
                off += (by_name[m].numel() + 3) // 4 * 4  # keep every view 16-byte aligned
        assert len(off_of) == len(self.params), "a pack's first member must come first in named_parameters order"
        self.offsets = [off_of[n] for n in self.names]
        self.numel = off
        self.packs = {}
        for key, names in (packs or {}).items():
            ms = [by_name[n] for n in names]
            rows = sum(m.shape[0] for m in ms)
            self.packs[key] = Pack(self, ms, (rows,) + tuple(ms[0].shape[1:]))
        self.flat = None
        self.pending = False
        self.on_ready = None  # optional callback(param) used by ddp.GradReducer
        self.cycle = None     # CycleState of micro-batched graph replays; None until a graph asks for it (cycle_state)
        self.gated = None     # the CycleState while a micro-stepped step body runs: the clear is gated, _adopt adds
        for p in self.params:
            p._mesm_gb = self
            # gradients that reach a parameter through plain autograd (tokens, embeddings used by
            # torch glue ops) are moved into the flat buffer as soon as they are accumulated
            p.register_post_accumulate_grad_hook(self._adopt)

    def _adopt(self, p):
        if self.flat is None:
            return
        g, v = p.grad, p._mesm_gview
        if g is None or g.data_ptr() == v.data_ptr():
            return
        p.grad = None  # let _open() see the pre-backward state of this parameter
        if self.pending:
            self._open()
        if self.gated is not None:
            v.add_(g)  # (a micro-step after the first of its cycle: the view holds the earlier micro-batches' sum)
        else:
            v.copy_(g)  # (overwrites the whole view: no zero fill in front of it)
        p.grad = v
        if self.on_ready is not None:
            self.on_ready(p)

    def ensure(self, device):
        if self.flat is not None and self.flat.device == device:
            return
        self.flat = torch.zeros(self.numel, device=device, dtype=torch.float32)
        for p, off in zip(self.params, self.offsets):
            p._mesm_gview = self.flat[off:off + p.numel()].view(p.shape)
            if p.grad is not None:
                p.grad = None

    def cycle_state(self, device):
        """the model's CycleState, made on first use (a model that never micro-steps holds none)"""
        self.ensure(device)
        if self.cycle is None or self.cycle.words.device != self.flat.device:
            self.cycle = CycleState(self.flat.device)
        return self.cycle

    def begin_step(self):
        self.pending = True

    def _open(self):
        self.pending = False
        if all(p.grad is None for p in self.params):
            if self.gated is not None:
                from . import kernels as kn
                kn.fill_zero_gated(self.flat, self.gated.phase_word)  # (cleared on the first replay of a cycle only)
            else:
                _zero(self.flat)
        else:
            for p in self.params:
                if p.grad is None:
                    p._mesm_gview.zero_()

    def acquire(self, p):
        """View to ACCUMULATE p's gradient into; makes p.grad alias it."""
        if self.pending:
            self._open()
        v = p._mesm_gview
        g = p.grad
        if g is None:
            p.grad = v
        elif g.data_ptr() != v.data_ptr():
            v.copy_(g)
            p.grad = v
        if self.on_ready is not None:
            _touched.append(p)  # reported by flush_ready() once the writing kernels are enqueued
        return v

    def zero(self):
        if self.flat is not None:
            _zero(self.flat)

    def attach_all(self):
        """Point every parameter's .grad at its view (used by graph-captured steps)."""
        for p in self.params:
            p.grad = p._mesm_gview


_touched = []


def flush_ready():
    """Called at the end of every backward block: the kernels that accumulate into the views
    handed out since the last flush are now enqueued, so a reducer may order a collective after them."""
    while _touched:
        p = _touched.pop()
        gb = p._mesm_gb
        if gb.on_ready is not None:
            gb.on_ready(p)


def grad_target(p):
    """(tensor to accumulate into, direct) for a parameter-like tensor.  `direct` means the
    tensor aliases p.grad and autograd must receive None for it."""
    gb = getattr(p, "_mesm_gb", None)
    if gb is not None and gb.flat is not None:
        return gb.acquire(p), True
    return torch.zeros_like(p), False
