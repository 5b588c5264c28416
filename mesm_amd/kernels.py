"""Tensor-level wrappers over the C-ABI (no autograd here; see ops.py).

Every function launches on torch's current HIP stream and returns immediately.
Tensors must live on the GPU, be fp32 and (unless stated) contiguous.  The one exception: the x of the LayerNorm
wrappers may be float16 (raw video features, FEATURE_DTYPES).
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import (ACT_NONE, ACT_PRELU, ACT_RELU, LAYOUT_OUTER_CONTIG,
                   LAYOUT_REDUCE_CONTIG, MASK_CAUSAL, MASK_KPAD, MASK_T2V_QUIRK, AttnArgs, GemmArgs, LnArgs,
                   check, lib, ptr, require_gpu, stream_ptr)

__all__ = [
    "gemm", "gemm_group", "layernorm_fwd", "layernorm_bwd", "attn_fwd", "attn_bwd", "sine_pos",
    "query_sine_fwd", "query_sine_bwd", "dropout", "act_bias_bwd",
    "ACT_NONE", "ACT_RELU", "ACT_PRELU",
]


# what raw input features may be stored as (model.forward's video_feat, the x of layernorm_fwd / layernorm_bwd)
FEATURE_DTYPES = (torch.float32, torch.float16)
MESM_EALIGN = -2


def _ln_dtypes(x, **f32):
    """TypeError before any launch: among floating tensors the LayerNorm kernels read float32, or float16 for x only (a
    tensor of another type would be misread through its address)."""
    if x.dtype not in FEATURE_DTYPES:
        raise TypeError("LayerNorm x must be float32 or float16 (mesm_amd.FEATURE_DTYPES), got %s" % x.dtype)
    for name, t in f32.items():
        if t is not None and t.dtype != torch.float32:
            raise TypeError("LayerNorm %s must be float32 (only x may also be float16), got %s" % (name, t.dtype))
    return x.dtype == torch.float16


# Device scalar (uint32 stored in an int32 tensor) added to every dropout seed at run time;
# set by graphed steps so that replays draw fresh masks.  None = no offset.
_seed_offset = None


def set_seed_offset(t):
    global _seed_offset
    if t is not None:
        assert t.is_cuda and t.dtype == torch.int32 and t.numel() == 1
    _seed_offset = t


def _seed_off_ptr():
    return _seed_offset.data_ptr() if _seed_offset is not None else None


class ZeroPool:
    """Zero-initialised scratch of one step out of ONE buffer that ONE fill clears when the step begins (MESM._begin):
    the gradient tensors that kernels accumulate into atomically (dq of an attention backward over several key tiles,
    token gradients, ...) used to be ~20 `torch.zeros` fill launches per step.  Sizes are learnt on the first step
    (served by plain torch.zeros, like anything that does not fit later); buffers that were ever handed out stay
    referenced, so HIP graphs captured against them keep valid addresses when the pool grows.
    Round 5: a second buffer for tensors of which only the LAST ROWS start at zero (`tail_zeroed`: the GEMM outputs of
    4800 / 4864 rows whose remainder tiles are split along K and meet by atomic adds, gemm()).  Which ranges those are is
    learnt like the sizes -- a step's requests are the ranges the NEXT step's fill clears -- and the one fill launch of the
    step (mesm_fill_ranges) clears the pool and those ranges together."""

    def __init__(self):
        self.buf, self.off, self.asked, self.retired = None, 0, 0, []
        self.part, self.poff, self.pasked = None, 0, 0
        self.cleared, self.wanted = set(), []  # (offset, length) float ranges of `part`: cleared by this step's fill / asked in it
        self.active = False  # between begin() and the next forward without one (MESM._begin: no-grad forwards do not fill)
        self.handed = {}     # data_ptr -> (cut, rows) of the tail-zeroed tensors handed out in THIS step, until a GEMM takes them
        # FORWARD activations live in the pool too (deep_out / rows_out with fwd=True: outputs that later blocks save for
        # their backward).  `fwd_live`: such tensors were handed out and no backward has reached the model's input side
        # since (MESM._forward hooks its first projection's gradient).  A begin() in that state -- a second grad-enabled
        # forward before the first one's backward: deferred backward, two models in one process -- must not clear or
        # re-issue those buffers: it lets go of them (the saved tensors keep their storage alive) and the step is served by
        # plain allocations; the next step gets fresh buffers.  Buffers a HIP graph was captured against are never freed.
        self.fwd_live = False
        self.in_graphs = False
        self.let_go = 0

    def idle(self):
        self.active = False
        self.handed = {}

    def backward_reached_inputs(self):
        self.fwd_live = False

    def _release(self):
        """drop this step's buffers without touching their contents (see fwd_live)"""
        for name in ("buf", "part"):
            b = getattr(self, name)
            if b is not None and self.in_graphs:
                self.retired.append(b)
            setattr(self, name, None)
        self.in_graphs = False
        self.cleared, self.wanted = set(), []
        self.let_go += 1

    def begin(self, device):
        capturing = torch.cuda.is_current_stream_capturing() if device.type == "cuda" else False
        if self.fwd_live and not capturing:
            self._release()
        self.fwd_live = False
        if capturing:
            self.in_graphs = True
        want = self.asked
        if want > 0 and (self.buf is None or self.buf.numel() < want or self.buf.device != device):
            if self.buf is not None:
                self.retired.append(self.buf)
            self.buf = torch.empty(want + want // 8, device=device, dtype=torch.float32)
        self.off = self.asked = 0
        want = self.pasked
        ranges = self.wanted
        if want > 0 and (self.part is None or self.part.numel() < want or self.part.device != device):
            if self.part is not None:
                self.retired.append(self.part)
            self.part = torch.empty(want + want // 8, device=device, dtype=torch.float32)
        if self.part is None or self.part.device != device:
            ranges = []
        self.poff = self.pasked = 0
        self.active = True
        self.handed = {}
        self.cleared, self.wanted = set(ranges), []
        todo = [(self.buf, 0, self.buf.numel())] if self.buf is not None else []
        todo += [(self.part, o, n) for o, n in ranges]
        if len(todo) == 1 and self.buf is not None:
            self.buf.zero_()
        elif todo:
            for k in range(0, len(todo), 32):
                chunk = todo[k:k + 32]
                ptrs = (ctypes.c_void_p * len(chunk))(*[t.data_ptr() + 4 * o for t, o, _ in chunk])
                nb = (ctypes.c_int64 * len(chunk))(*[4 * n for _, _, n in chunk])
                check(lib().mesm_fill_ranges(ptrs, nb, len(chunk), stream_ptr()), "mesm_fill_ranges")

    def zeros(self, shape, device):
        n = 1
        for d_ in shape:
            n *= int(d_)
        span = (n + 63) // 64 * 64  # 256-byte granules: every view is aligned for the vector paths
        self.asked += span
        if self.buf is not None and self.buf.device == device and self.off + span <= self.buf.numel():
            v = self.buf[self.off:self.off + n].view(shape)
            self.off += span
            return v
        return torch.zeros(shape, device=device, dtype=torch.float32)

    def serves(self, n, device):
        """would zeros() of n elements come out of the pool (no fill launch of its own)?  If not, the request is still
        counted, so that the next step's pool has room for it."""
        span = (n + 63) // 64 * 64
        ok = self.buf is not None and self.buf.device == device and self.off + span <= self.buf.numel()
        if not ok:
            self.asked += span
        return ok

    def tail_zeroed(self, shape, cut, device):
        """fp32 (rows, cols) tensor whose rows [cut, rows) are zero when the step reaches it (the rows above: anything).
        -> (tensor, True), or (None, False) when the pool cannot serve it in this step (first step of a shape, ...)."""
        rows, cols = int(shape[0]), int(shape[1])
        n = rows * cols
        span = (n + 63) // 64 * 64
        off = self.poff
        rng = (off + cut * cols, (rows - cut) * cols)
        self.pasked += span
        self.poff += span
        self.wanted.append(rng)
        if (cut * cols) % 4 or ((rows - cut) * cols) % 4:
            return None, False
        if self.part is not None and self.part.device == device and off + span <= self.part.numel() and rng in self.cleared:
            self.cleared.discard(rng)  # (handed out once per fill)
            return self.part[off:off + n].view(rows, cols), True
        return None, False


zero_pool = ZeroPool()


def fill_zero(t):
    """t (contiguous, 16-byte aligned, a multiple of 16 bytes) <- 0 in one launch of the library's own fill"""
    ptrs = (ctypes.c_void_p * 1)(t.data_ptr())
    nb = (ctypes.c_int64 * 1)(t.numel() * t.element_size())
    check(lib().mesm_fill_ranges(ptrs, nb, 1, stream_ptr()), "mesm_fill_ranges")


def fill_zero_gated(t, phase):
    """fill_zero(t) iff the device word `phase` (int32) is 0 when the launch runs; otherwise nothing is written"""
    assert phase.is_cuda and phase.dtype == torch.int32
    ptrs = (ctypes.c_void_p * 1)(t.data_ptr())
    nb = (ctypes.c_int64 * 1)(t.numel() * t.element_size())
    check(lib().mesm_fill_ranges_gated(ptrs, nb, 1, ptr(phase), stream_ptr()), "mesm_fill_ranges_gated")


def micro_begin(state, seed_ctr=None):
    """first node of a micro-stepped graph (one thread): the four cycle words {count, k, phase, due} move on to this
    replay and the dropout seed offset advances (csrc/glue.hip: micro_begin_kernel)"""
    assert state.is_cuda and state.dtype == torch.int32 and state.numel() == 4 and state.is_contiguous()
    check(lib().mesm_micro_begin(ptr(state), ptr(seed_ctr), stream_ptr()), "mesm_micro_begin")


def zeros(shape, device):
    """fp32 zeros that live until the next step begins (see ZeroPool)"""
    return zero_pool.zeros(tuple(shape), device)


ROW_CUT = 4096  # rows of one full round of 64 x 64 tiles on 256 CUs at 256 columns (gemm(): _SPLIT_ROWS)


_DEEP_K = int(os.environ.get("MESM_GEMM_DEEP_K", "768"))        # products this deep with few tiles are split along K (0: off)
_DEEP_DEPTH = int(os.environ.get("MESM_GEMM_DEEP_DEPTH", "256"))  # reduce indices per workgroup they aim at


# forward products onto pool-zeroed outputs by atomic adds make the ACTIVATIONS differ in the last bit from run to run; a
# ReLU / PReLU kink or a dropped / kept boundary that flips on such a bit moves the step's gradient by a few 1e-5 of its norm
# (tools/probe/run_to_run.py).  0: only backward products are split that way (gradients then differ at the 1e-7 level).
_FWD_ATOMICS = os.environ.get("MESM_GEMM_FWD_ATOMICS", "1") == "1"


def deep_out(shape, K, device, fwd=False):
    """Output tensor (fp32) of a product with K reduce indices and a LINEAR epilogue.  Few tiles x a deep reduce range --
    320 x 256 x 1024 in the decoder's FFN, 1024 x 256 x 5003 behind the vocabulary head -- is a handful of workgroups that walk
    16-80 stages each while the chip idles, and inside a grouped launch they are what the launch waits for.  Such an output
    comes from the step's zero pool (cleared by the one fill launch) and gemm() splits the product along K, partial sums by
    atomic adds; anything else gets a plain uninitialised tensor."""
    shape = tuple(int(d_) for d_ in shape)
    cols = shape[-1]
    rows = 1
    for d_ in shape[:-1]:
        rows *= d_
    t64 = ((rows + 63) // 64) * ((cols + 63) // 64)
    if (zero_pool.active and _DEEP_K > 0 and (_FWD_ATOMICS or not fwd) and K >= _DEEP_K and t64 <= 128
            and min(K // _DEEP_DEPTH, 256 // t64) >= 2 and zero_pool.serves(rows * cols, device)):
        t = zero_pool.zeros(shape, device)
        zero_pool.handed[t.data_ptr()] = (0, rows)  # (gemm() takes it: every row starts at zero)
        zero_pool.fwd_live = zero_pool.fwd_live or fwd
        return t
    return torch.empty(shape, device=device, dtype=torch.float32)


def rows_out(like, K=0, fwd=False):
    """Output tensor of a GEMM with like.shape: when it is one of the 4800 / 4864-row x 256-column products whose remainder
    rows gemm() runs split along K, a tensor whose remainder rows start at zero (ZeroPool.tail_zeroed); a small output of a
    deep product (K given): deep_out; else empty_like."""
    cols = like.shape[-1]
    rows = like.numel() // cols
    if fwd and not _FWD_ATOMICS:
        return torch.empty_like(like)
    if K and rows <= ROW_CUT:
        return deep_out(like.shape, K, like.device, fwd)
    if (_SPLIT_ROWS and _SPLIT_TAIL > 1 and cols == 256 and ROW_CUT < rows <= 5120 and like.dtype == torch.float32
            and zero_pool.active):  # (the pool's fill runs at the start of a TRAINING step, MESM._begin)
        t, ok = zero_pool.tail_zeroed((rows, cols), ROW_CUT, like.device)
        if ok:
            zero_pool.handed[t.data_ptr()] = (ROW_CUT, rows)  # (gemm() takes it: valid for one product of this step)
            zero_pool.fwd_live = zero_pool.fwd_live or fwd
            return t.view(like.shape)
    return torch.empty_like(like)


def _mat(t):
    """(rows, cols, ld, layout_if_reduce_is_cols) view info of a 2-D tensor with one unit stride."""
    assert t.dim() == 2
    r, c = t.shape
    s0, s1 = t.stride()
    return r, c, s0, s1


def gemm_switches(tile=None, bf16x=None):
    """tuning tools: flip the GEMM dispatch switches (MESM_GEMM_TILE / MESM_GEMM_BF16X, otherwise read once at load)"""
    check(lib().mesm_gemm_set_switches(-1 if tile is None else int(tile), -1 if bf16x is None else int(bf16x)),
          "mesm_gemm_set_switches")


def gemm_mode():
    """the GEMM arithmetic in force: 6 = three-term bf16 split, 2 = two-term fp16 split, 0 = exact f32 MFMA"""
    return int(lib().mesm_gemm_get_bf16x())


def gemm(A, B, C, *, trans_a=False, trans_b=False, A2=None, B2=None, bias=None, residual=None,
         aux=None, slope=None, dslope=None, colsum=None, a_act=ACT_NONE, b_act=ACT_NONE,
         a_drop=(0.0, 0), b_drop=(0.0, 0), e_act=ACT_NONE, e_actgrad=ACT_NONE,
         e_drop=(0.0, 0), out_scale=1.0, accumulate=0, split_k=1, pre_out=None, row0=0):
    """C[M,N] (+)= epi( op(A) @ op(B) ).

    A is (M,K) (or (K,M) with trans_a), B is (K,N) (or (N,K) with trans_b); both are
    2-D views whose last stride is 1.  C is (M,N) with unit column stride.
    """
    require_gpu(A, B, C)
    if (_SPLIT_ROWS and row0 == 0 and not trans_a and C.shape[1] == 256 and A.shape[1] >= 1024
            and 4096 < C.shape[0] <= 5120 and split_k == 1 and colsum is None and dslope is None and A2 is None
            and float(a_drop[0]) == 0.0 and a_act == ACT_NONE):
        # 4800 / 4864-row outputs of width 256: 300 tiles of 64 x 64 on 256 CUs are two rounds with the second 17 %
        # full.  Rows [0, 4096) = 256 tiles = exactly one round of the k-split 64 x 64 kernel; the remainder goes
        # to the 32 x 32 kernel (4800 x 256 x 1024: 37 us -> 30 us).  The epilogue-dropout mask index carries the
        # row offset, every other epilogue term is row-local.
        cut = ROW_CUT
        sl = lambda t_, a_, b_: None if t_ is None else t_[a_:b_]
        # the remainder's 44 / 48 tiles alone are a second, mostly empty round: when its rows of C start at zero (rows_out)
        # and the epilogue is linear, they are split along K as well -- 4 x as many workgroups, partial sums by atomic adds
        # (bias / residual join the first slice, every slice applies the same dropout mask): 28.5 -> 21.8 us at 4800 rows
        tail = (zero_pool.handed.pop(C.data_ptr(), None) == (cut, C.shape[0]) and accumulate == 0 and e_act == ACT_NONE
                and e_actgrad == ACT_NONE and pre_out is None and B2 is None and C.is_contiguous())
        for lo, hi in ((0, cut), (cut, C.shape[0])):
            gemm(A[lo:hi], B, C[lo:hi], trans_b=trans_b, B2=B2, bias=bias, residual=sl(residual, lo, hi),
                 aux=sl(aux, lo, hi), slope=slope, a_act=a_act, b_act=b_act, a_drop=a_drop, b_drop=b_drop,
                 e_act=e_act, e_actgrad=e_actgrad, e_drop=e_drop, out_scale=out_scale, accumulate=accumulate,
                 pre_out=sl(pre_out, lo, hi), row0=lo if lo else -1, split_k=_SPLIT_TAIL if (tail and lo) else 1)
        return C
    row0 = max(row0, 0)
    if zero_pool.handed and zero_pool.handed.get(C.data_ptr()) == (0, C.shape[0]):
        # an output from deep_out(): every row starts at zero -- few tiles, a deep reduce range, a linear epilogue: split along K
        zero_pool.handed.pop(C.data_ptr())
        Kd = A.shape[0] if trans_a else A.shape[1]
        t64 = ((C.shape[0] + 63) // 64) * ((C.shape[1] + 63) // 64)
        if (split_k == 1 and accumulate == 0 and e_act == ACT_NONE and e_actgrad in (ACT_NONE, ACT_RELU) and pre_out is None
                and C.is_contiguous()):
            split_k = max(1, min(Kd // _DEEP_DEPTH, 256 // t64, 16))
    assert A.dtype == B.dtype == C.dtype == torch.float32
    assert A.dim() == 2 and B.dim() == 2 and C.dim() == 2
    assert A.stride(1) == 1 and B.stride(1) == 1 and C.stride(1) == 1
    if trans_a:
        K, M = A.shape
        a_layout = LAYOUT_OUTER_CONTIG  # element (m, k) at k*ld + m
    else:
        M, K = A.shape
        a_layout = LAYOUT_REDUCE_CONTIG
    if trans_b:
        N, Kb = B.shape
        b_layout = LAYOUT_REDUCE_CONTIG  # element (n, k) at n*ld + k
    else:
        Kb, N = B.shape
        b_layout = LAYOUT_OUTER_CONTIG
    assert K == Kb, (A.shape, B.shape, trans_a, trans_b)
    assert C.shape == (M, N), (C.shape, M, N)
    g = GemmArgs()
    g.A, g.B, g.C = A.data_ptr(), B.data_ptr(), C.data_ptr()
    if A2 is not None:
        assert A2.shape == A.shape and A2.stride() == A.stride()
        g.A2 = A2.data_ptr()
    if B2 is not None:
        assert B2.shape == B.shape and B2.stride() == B.stride()
        g.B2 = B2.data_ptr()
    g.M, g.N, g.K = M, N, K
    g.a_layout, g.b_layout = a_layout, b_layout
    g.lda, g.ldb, g.ldc = A.stride(0), B.stride(0), C.stride(0)
    if bias is not None:
        assert bias.numel() == N and bias.is_contiguous()
        g.bias = bias.data_ptr()
    if residual is not None:
        assert residual.shape == (M, N) and residual.stride(1) == 1
        g.residual, g.ldr = residual.data_ptr(), residual.stride(0)
    if aux is not None:
        assert aux.shape == (M, N) and aux.stride(1) == 1
        g.aux, g.ldaux = aux.data_ptr(), aux.stride(0)
    if slope is not None:
        g.slope = slope.data_ptr()
    if dslope is not None:
        g.dslope = dslope.data_ptr()
        # one partial per workgroup of the finest tiling; stream-ordered scratch
        ws = torch.empty(((M + 31) // 32) * ((N + 31) // 32) * max(int(split_k), 1), device=C.device,
                         dtype=torch.float32)
        g.dslope_ws = ws.data_ptr()
    if colsum is not None:
        assert colsum.numel() == M
        g.colsum = colsum.data_ptr()
    g.a_act, g.b_act = a_act, b_act
    g.a_drop_p, g.a_drop_seed = float(a_drop[0]), int(a_drop[1]) & 0xFFFFFFFF
    g.b_drop_p, g.b_drop_seed = float(b_drop[0]), int(b_drop[1]) & 0xFFFFFFFF
    g.e_act, g.e_actgrad = e_act, e_actgrad
    _check_drop_index(M * N, float(e_drop[0]))
    _check_drop_index(M * K, float(a_drop[0]))
    _check_drop_index(N * K, float(b_drop[0]))
    g.e_drop_p, g.e_drop_seed = float(e_drop[0]), int(e_drop[1]) & 0xFFFFFFFF
    g.out_scale = float(out_scale)
    g.accumulate, g.split_k = int(accumulate), int(split_k)
    if pre_out is not None:
        assert pre_out.shape == (M, N) and pre_out.stride(1) == 1
        g.pre_out, g.ldpre = pre_out.data_ptr(), pre_out.stride(0)
    g.e_drop_row0 = int(row0)
    g.seed_offset = _seed_off_ptr()
    if _phase is not None:
        # inside a launch phase: queued; the tensors stay referenced until the phase is launched
        _phase.add("gemm", g, (A, B, C, A2, B2, bias, residual, aux, slope, dslope, colsum,
                               ws if dslope is not None else None, pre_out))
        return C
    check(lib().mesm_gemm_f32(ctypes.byref(g), stream_ptr()), "mesm_gemm_f32")
    if dslope is not None:
        _side_keep.append(ws)
        gemm_flush_side()  # a direct call: nothing is known about a following launch
    return C


_SPLIT_ROWS = os.environ.get("MESM_GEMM_SPLIT_ROWS", "1") == "1"
_SPLIT_TAIL = int(os.environ.get("MESM_GEMM_SPLIT_TAIL", "4"))  # k-slices of the remainder rows (1: off)


class _Phase:
    """Launches queued by kind; `flush` issues every kind through its grouped entry point."""
    KINDS = (("gemm", GemmArgs, "mesm_gemm_group", "mesm_gemm_f32"),
             ("ln_fwd", LnArgs, "mesm_layernorm_fwd_group", None),
             ("ln_fwd_xh", LnArgs, "mesm_layernorm_fwd_group_xh", None),  # float16 x: lists of their own
             ("ln_bwd", LnArgs, "mesm_layernorm_bwd_group", None),
             ("ln_bwd_xh", LnArgs, "mesm_layernorm_bwd_group_xh", None),
             ("attn_fwd", AttnArgs, "mesm_attn_fwd_group", "mesm_attn_fwd"),
             ("attn_bwd", AttnArgs, "mesm_attn_bwd_group", "mesm_attn_bwd"),
             ("glue", _lib.GlueArgs, "mesm_glue_group", None))

    def __init__(self):
        self.q = {k[0]: [] for k in self.KINDS}
        self.keep = []

    def add(self, kind, args, keep):
        self.q[kind].append(args)
        self.keep.append(keep)

    def flush(self):
        L, st = lib(), stream_ptr()
        for kind, struct, group_fn, single_fn in self.KINDS:
            items = self.q[kind]
            for i in range(0, len(items), 64):
                chunk = items[i:i + 64]
                if len(chunk) == 1 and single_fn is not None:
                    check(getattr(L, single_fn)(ctypes.byref(chunk[0]), st), single_fn)
                    continue
                arr = (struct * len(chunk))(*chunk)
                check(getattr(L, group_fn)(arr, len(chunk), st), group_fn)
            self.q[kind] = []
        # the workspaces of slope-gradient partials are read by a LATER launch (the reduction rides in the next GEMM
        # launch of the stream, gemm.hip side_reduce): keep them until gemm_flush_side() at the end of the block
        _side_keep.extend(self.keep)
        self.keep = []


_phase = None
_side_keep = []
_side_defer = 0


def defer_side(d):
    """ops._drive brackets a block's phases with +1 / -1: inside, a phase end leaves pending slope-gradient reductions
    to the next phase's GEMM launches; a phase used on its own (gemm_group in user code) completes them on exit."""
    global _side_defer
    _side_defer += d


def gemm_flush_side():
    """Slope-gradient reductions that no GEMM launch has picked up yet get their own launch; called at the end of every
    backward block (ops._drive) and after a direct gemm(..., dslope=...) call."""
    check(lib().mesm_gemm_flush_side(stream_ptr()), "mesm_gemm_flush_side")
    _side_keep.clear()


def gemm_drop_side():
    """error path: pending reductions are forgotten, not run (their workspaces are released with the failed block)"""
    lib().mesm_gemm_drop_side()
    _side_keep.clear()


class phase:
    """Context manager: ONE LAUNCH PHASE.  The gemm / layernorm / attention calls made inside are INDEPENDENT of
    each other (none reads what another writes; atomic accumulation into the same gradient view is fine); they
    are queued and issued together on exit, every kind through its grouped entry point (mesm_gemm_group,
    mesm_layernorm_*_group, mesm_attn_*_group): problems of one kind share launches of up to 8.  Kernels of other
    kinds called inside run immediately, i.e. BEFORE the queued ones.  Nothing may be enqueued inside the block
    that consumes the outputs of a queued launch.  Nested phases join the outermost one."""

    def __enter__(self):
        global _phase
        self.outer = _phase
        if _phase is None:
            _phase = _Phase()
        return self

    def __exit__(self, et, ev, tb):
        global _phase
        if self.outer is not None:  # nested: the outermost phase launches
            return False
        ph, _phase = _phase, None
        if et is not None:
            gemm_drop_side()  # the workspaces of pending slope-gradient reductions die with the failed block
            return False
        try:
            ph.flush()
            if _side_defer == 0:
                gemm_flush_side()
        except BaseException:
            gemm_drop_side()
            raise
        return False


gemm_group = phase  # the older name: a phase that only holds GEMMs


def layernorm_fwd(x, gamma, beta, eps=1e-5, drop=(0.0, 0), add=None, out=None):
    """y = dropout(LN(x)) (drop = (p, seed); p = 0: plain LayerNorm), mean, rstd.
    add (same shape as x): also return y + add as a fourth value (one extra store stream).
    out: where y is written (a contiguous tensor of x's size, e.g. a slot of a stacked output).
    x may be float16 (raw features): y, mean and rstd are float32 all the same, bit for bit what x.float() gives; no
    `add` in that form."""
    require_gpu(x, gamma, beta)
    xh = _ln_dtypes(x, gamma=gamma, beta=beta, add=add, out=out)
    if xh and add is not None:
        raise TypeError("layernorm_fwd: a float16 x takes no `add` (float32 only)")
    D = x.shape[-1]
    x2 = x.reshape(-1, D)
    assert x2.is_contiguous()
    rows = x2.shape[0]
    if out is not None:
        assert out.is_contiguous() and out.numel() == x2.numel() and out.dtype == torch.float32 and out.device == x2.device
        y = out.view(rows, D)
    else:
        y = torch.empty(x2.shape, device=x2.device, dtype=torch.float32)
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    _check_drop_index(x2.numel(), float(drop[0]))
    y2 = None
    if add is not None:
        assert add.is_contiguous() and add.numel() == x2.numel()
        y2 = torch.empty_like(x2)
    if xh and _phase is not None and x2.data_ptr() % 8:
        x2 = x2.clone()  # (a queued launch cannot be retried: what MESM_EALIGN would say is checked here)
    if _phase is not None or xh:
        a = LnArgs()
        a.x, a.gamma, a.beta, a.y, a.mean, a.rstd = (x2.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                                                     mean.data_ptr(), rstd.data_ptr())
        a.rows, a.D, a.eps = rows, D, float(eps)
        a.drop_p, a.drop_seed, a.seed_offset = float(drop[0]), int(drop[1]) & 0xFFFFFFFF, _seed_off_ptr()
        if add is not None:
            a.add, a.y2 = add.data_ptr(), y2.data_ptr()
        if xh and _phase is None:
            rc = lib().mesm_layernorm_fwd_group_xh(ctypes.byref(a), 1, stream_ptr())
            if rc == MESM_EALIGN:  # a view that starts off an 8-byte boundary: nothing was launched; a fresh copy is aligned
                x2 = x2.clone()
                a.x = x2.data_ptr()
                rc = lib().mesm_layernorm_fwd_group_xh(ctypes.byref(a), 1, stream_ptr())
            check(rc, "mesm_layernorm_fwd_group_xh")
            return y.view(x.shape), mean, rstd
        _phase.add("ln_fwd_xh" if xh else "ln_fwd", a, (x2, gamma, beta, y, mean, rstd, add, y2))
        if add is not None:
            return y.view(x.shape), mean, rstd, y2.view(x.shape)
        return y.view(x.shape), mean, rstd
    check(lib().mesm_layernorm_fwd2(ptr(x2), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd),
                                    rows, D, eps, float(drop[0]), int(drop[1]) & 0xFFFFFFFF,
                                    ptr(_seed_offset), ptr(add), ptr(y2), stream_ptr()), "mesm_layernorm_fwd2")
    if add is not None:
        return y.view(x.shape), mean, rstd, y2.view(x.shape)
    return y.view(x.shape), mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta, dx=None, accumulate_dx=False, need_dx=True,
                  drop=(0.0, 0), drop2=None, dyb=None, addend=None, relu_in=False):
    """dgamma/dbeta are ACCUMULATED into (flat-gradient views).  need_dx=False: parameter
    gradients only (returns None).  drop: the (p, seed) the forward fused; dy is masked on load.
    drop2 = (p, seed): also return dropout(dx; p, seed) as a second tensor -> (dx, dx2).
    dyb: gradient of a second consumer of y (added to dy on load); addend: a gradient reaching x on
    another route (added to dx on store)."""
    dp, dseed = float(drop[0]), int(drop[1]) & 0xFFFFFFFF
    require_gpu(dy, x, gamma)
    xh = _ln_dtypes(x, dy=dy, gamma=gamma, mean=mean, rstd=rstd, dgamma=dgamma, dbeta=dbeta, dx=dx, dyb=dyb, addend=addend)
    if xh and (need_dx or drop2 is not None or dyb is not None or addend is not None or relu_in):
        raise TypeError("layernorm_bwd: a float16 x is raw input features and carries no gradient -- need_dx=False only "
                        "(dx, drop2, dyb, addend, relu_in want a float32 x)")
    D = x.shape[-1]
    x2 = x.reshape(-1, D)
    dy2 = dy.reshape(-1, D)
    assert x2.is_contiguous() and dy2.is_contiguous()
    assert not relu_in or (need_dx and D <= 512)
    if (_phase is not None or xh) and not need_dx and drop2 is None and dyb is None and addend is None:
        # parameter gradients only: a small problem (the 512-d word / sentence inputs) rides in the phase's grouped launch,
        # two wide ones over the same x (the raw video features' twin LayerNorms) share one pass over x
        a = LnArgs()
        a.dy, a.x, a.gamma, a.mean, a.rstd = dy2.data_ptr(), x2.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr()
        a.dgamma, a.dbeta = dgamma.data_ptr(), dbeta.data_ptr()
        a.rows, a.D = x2.shape[0], D
        a.drop_p, a.drop_seed, a.seed_offset = dp, dseed, _seed_off_ptr()
        if _phase is None:
            check(lib().mesm_layernorm_bwd_group_xh(ctypes.byref(a), 1, stream_ptr()), "mesm_layernorm_bwd_group_xh")
            return None
        _phase.add("ln_bwd_xh" if xh else "ln_bwd", a, (dy2, x2, gamma, mean, rstd, dgamma, dbeta))
        return None
    if (_phase is not None or relu_in) and need_dx:
        for t_ in (dyb, addend):
            assert t_ is None or (t_.is_contiguous() and t_.numel() == x2.numel())
        if dx is None:
            assert not accumulate_dx
            dx = torch.empty_like(x2)
        dxv = dx.view(-1, D)
        dxm = torch.empty_like(dxv) if drop2 is not None else None
        a = LnArgs()
        a.dy, a.x, a.gamma, a.mean, a.rstd = dy2.data_ptr(), x2.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr()
        a.dx, a.dgamma, a.dbeta = dxv.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr()
        a.rows, a.D = x2.shape[0], D
        a.accumulate_dx = 1 if accumulate_dx else 0
        a.drop_p, a.drop_seed, a.seed_offset = dp, dseed, _seed_off_ptr()
        if drop2 is not None:
            a.dx2, a.drop2_p, a.drop2_seed = dxm.data_ptr(), float(drop2[0]), int(drop2[1]) & 0xFFFFFFFF
        if dyb is not None:
            a.dyb = dyb.data_ptr()
        if addend is not None:
            a.addend = addend.data_ptr()
        a.relu_in = 1 if relu_in else 0
        if _phase is not None:
            _phase.add("ln_bwd", a, (dy2, x2, gamma, mean, rstd, dxv, dgamma, dbeta, dxm, dyb, addend))
        else:
            check(lib().mesm_layernorm_bwd_group(ctypes.byref(a), 1, stream_ptr()), "mesm_layernorm_bwd_group")
        return (dxv.view(x.shape), dxm.view(x.shape)) if drop2 is not None else dxv.view(x.shape)
    if dyb is not None or addend is not None:
        assert need_dx
        for t_ in (dyb, addend):
            assert t_ is None or (t_.is_contiguous() and t_.numel() == x2.numel())
        if dx is None:
            dx = torch.empty_like(x2)
        dxv = dx.view(-1, D)
        dxm = torch.empty_like(dxv) if drop2 is not None else None
        check(lib().mesm_layernorm_bwd3(ptr(dy2), ptr(x2), ptr(gamma), ptr(mean), ptr(rstd), ptr(dxv),
                                        ptr(dgamma), ptr(dbeta), x2.shape[0], D, 1 if accumulate_dx else 0, dp, dseed,
                                        ptr(_seed_offset), ptr(dxm), float(drop2[0]) if drop2 else 0.0,
                                        (int(drop2[1]) & 0xFFFFFFFF) if drop2 else 0, ptr(dyb), ptr(addend),
                                        stream_ptr()), "mesm_layernorm_bwd3")
        return (dxv.view(x.shape), dxm.view(x.shape)) if drop2 is not None else dxv.view(x.shape)
    if not need_dx:
        assert drop2 is None
        check(lib().mesm_layernorm_bwd(ptr(dy2), ptr(x2), ptr(gamma), ptr(mean), ptr(rstd), None,
                                       ptr(dgamma), ptr(dbeta), x2.shape[0], D, 0, dp, dseed,
                                       ptr(_seed_offset), stream_ptr()),
              "mesm_layernorm_bwd")
        return None
    if dx is None:
        assert not accumulate_dx
        dx = torch.empty_like(x2)
    dx2 = dx.view(-1, D)
    if drop2 is None:
        check(lib().mesm_layernorm_bwd(ptr(dy2), ptr(x2), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx2),
                                       ptr(dgamma), ptr(dbeta), x2.shape[0], D,
                                       1 if accumulate_dx else 0, dp, dseed, ptr(_seed_offset), stream_ptr()),
              "mesm_layernorm_bwd")
        return dx2.view(x.shape)
    dxm = torch.empty_like(dx2)
    check(lib().mesm_layernorm_bwd2(ptr(dy2), ptr(x2), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx2),
                                    ptr(dgamma), ptr(dbeta), x2.shape[0], D,
                                    1 if accumulate_dx else 0, dp, dseed, ptr(_seed_offset), ptr(dxm),
                                    float(drop2[0]), int(drop2[1]) & 0xFFFFFFFF, stream_ptr()),
          "mesm_layernorm_bwd2")
    return dx2.view(x.shape), dxm.view(x.shape)


# Device scalar (int32) with the number of VALID pairs of a batch padded to a captured capacity (graphed.py sets it
# around the capture of a padded step): the modulus of the attention mask quirk.  None = the batch extent.
_mask_mod = None


def set_mask_mod(t):
    global _mask_mod
    if t is not None:
        assert t.is_cuda and t.dtype == torch.int32 and t.numel() == 1
    _mask_mod = t


def _attn_args(q, k, v, o, lse, H, kpad, qpad, scale, drop, group=0, causal=False, q2=None, k2=None, k_add=None):
    B, Lq, Eq = q.shape
    _, Lk, Ek = k.shape
    Ev = v.shape[2]
    assert Eq == Ek and Eq % H == 0 and Ev % H == 0
    for t in (q, k, v, o):
        assert t.dtype == torch.float32 and t.stride(2) == 1
    a = AttnArgs()
    a.q, a.k, a.v, a.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()
    a.lse = lse.data_ptr() if lse is not None else None
    if q2 is not None:  # split heads: [q || q2] per head (see MesmAttnArgs.q2)
        assert q2.shape == q.shape and q2.stride() == q.stride() and k2.shape == k.shape and k2.stride() == k.stride()
        a.q2, a.k2 = q2.data_ptr(), k2.data_ptr()
        if k_add is not None:
            assert k_add.shape == k.shape and k_add.stride() == k.stride()
            a.k_add = k_add.data_ptr()
        Eq *= 2
    a.B, a.H, a.Lq, a.Lk, a.dk, a.dv = B, H, Lq, Lk, Eq // H, Ev // H
    a.q_bs, a.q_ls = q.stride(0), q.stride(1)
    a.k_bs, a.k_ls = k.stride(0), k.stride(1)
    a.v_bs, a.v_ls = v.stride(0), v.stride(1)
    a.o_bs, a.o_ls = o.stride(0), o.stride(1)
    if kpad is not None:
        assert kpad.dtype in (torch.uint8, torch.bool) and kpad.shape == (B, Lk) and kpad.is_contiguous()
        a.kpad = kpad.data_ptr()
    if qpad is not None:
        assert qpad.dtype in (torch.uint8, torch.bool) and qpad.shape == (B, Lq) and qpad.is_contiguous()
        a.qpad = qpad.data_ptr()
        a.mask_mode = MASK_T2V_QUIRK
        if _mask_mod is not None:
            a.mask_mod = _mask_mod.data_ptr()
    else:
        a.mask_mode = MASK_KPAD
    if causal:
        assert qpad is None
        a.mask_mode = MASK_CAUSAL
    a.scale = float(scale)
    _check_drop_index(B * H * Lq * Lk, float(drop[0]))
    a.drop_p, a.drop_seed = float(drop[0]), int(drop[1]) & 0xFFFFFFFF
    a.seed_offset = _seed_off_ptr()
    a.mask_group = int(group)
    return a


def attn_fwd(q, k, v, H, kpad=None, qpad=None, scale=None, drop=(0.0, 0), group=0, causal=False, want_lse=True,
             q2=None, k2=None, k_add=None):
    """q (B,Lq,H*dk), k (B,Lk,H*dk), v (B,Lk,H*dv) -> o (B,Lq,H*dv), lse (B,H,Lq).
    causal: key j of query i is masked iff j > i (frozen CLIP text transformer; forward only).
    q2 / k2: split heads, the head's features are [q || q2] / [k || k2] (each half H*dk/2 columns)."""
    require_gpu(q, k, v)
    B, Lq, Eq = q.shape
    if q2 is not None:
        Eq *= 2
    if scale is None:
        scale = (Eq // H) ** -0.5
    o = torch.empty(B, Lq, v.shape[2], device=q.device, dtype=torch.float32)
    lse = torch.empty(B, H, Lq, device=q.device, dtype=torch.float32) if want_lse else None
    a = _attn_args(q, k, v, o, lse, H, kpad, qpad, scale, drop, group, causal, q2, k2, k_add)
    if _phase is not None:
        _phase.add("attn_fwd", a, (q, k, v, o, lse, kpad, qpad, q2, k2, k_add))
        return o, lse
    check(lib().mesm_attn_fwd(ctypes.byref(a), stream_ptr()), "mesm_attn_fwd")
    return o, lse


_dq_zero_cache = {}


def attn_bwd_adds_dq(B, H, Lq, Lk, dk, dv, split=False):
    """True where the attention backward that will run for this shape ADDS into dq (lane-per-key kernel, several key
    tiles): the caller hands in zeros (from the step's zero pool); the matrix-core paths write dq."""
    key = (int(B), int(H), int(Lq), int(Lk), int(dk), int(dv), 1 if split else 0)
    need = _dq_zero_cache.get(key)
    if need is None:
        need = _dq_zero_cache[key] = bool(lib().mesm_attn_bwd_accumulates_dq(*key))
    return need


def attn_bwd(do, q, k, v, o, lse, H, kpad=None, qpad=None, scale=None, drop=(0.0, 0), group=0, q2=None, k2=None):
    """-> dq, dk, dv (and dq2, dk2 with split heads)."""
    require_gpu(do, q, k, v, o, lse)
    B, Lq, Eq = q.shape
    if q2 is not None:
        Eq *= 2
    if scale is None:
        scale = (Eq // H) ** -0.5
    do = do.contiguous() if do.stride() != o.stride() else do
    assert do.stride() == o.stride()
    # dq is accumulated atomically when there are several key tiles -> start from zero
    dq = torch.zeros(q.shape, device=q.device, dtype=torch.float32)
    dk = torch.empty(k.shape, device=q.device, dtype=torch.float32)
    dv = torch.empty(v.shape, device=q.device, dtype=torch.float32)
    qc, kc, vc = q, k, v
    # gradients are written with the strides of q/k/v: require the packed layout
    assert q.is_contiguous() and k.is_contiguous() and v.is_contiguous()
    a = _attn_args(qc, kc, vc, o, lse, H, kpad, qpad, scale, drop, group, False, q2, k2)
    a.d_o, a.dq, a.dk_, a.dv_ = do.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    if q2 is not None:
        assert q2.is_contiguous() and k2.is_contiguous()
        dq2 = torch.zeros(q2.shape, device=q.device, dtype=torch.float32)
        dk2 = torch.empty(k2.shape, device=q.device, dtype=torch.float32)
        a.dq2, a.dk2 = dq2.data_ptr(), dk2.data_ptr()
    check(lib().mesm_attn_bwd(ctypes.byref(a), stream_ptr()), "mesm_attn_bwd")
    if q2 is not None:
        return dq, dk, dv, dq2, dk2
    return dq, dk, dv


def attn_bwd_into(do, q, k, v, o, lse, H, dq, dk, dv, kpad=None, qpad=None, scale=None,
                  drop=(0.0, 0), group=0, q2=None, k2=None, dq2=None, dk2=None, k_add=None):
    """attn_bwd writing into caller-provided gradient tensors whose strides equal those of
    q / k / v (e.g. column slices of one fused [dq|dk|dv] buffer).  dq must be zero-initialised
    when Lk > 64 (several key tiles add into it atomically)."""
    require_gpu(do, q, k, v, o, lse, dq, dk, dv)
    if scale is None:
        scale = ((q.shape[-1] * (2 if q2 is not None else 1)) // H) ** -0.5
    assert do.stride() == o.stride()
    assert dq.stride() == q.stride() and dk.stride() == k.stride() and dv.stride() == v.stride()
    a = _attn_args(q, k, v, o, lse, H, kpad, qpad, scale, drop, group, False, q2, k2, k_add)
    a.d_o, a.dq, a.dk_, a.dv_ = do.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    if q2 is not None:
        assert dq2.stride() == q.stride() and dk2.stride() == k.stride()
        a.dq2, a.dk2 = dq2.data_ptr(), dk2.data_ptr()
    if _phase is not None:
        _phase.add("attn_bwd", a, (do, q, k, v, o, lse, dq, dk, dv, kpad, qpad, q2, k2, dq2, dk2, k_add))
        return
    check(lib().mesm_attn_bwd(ctypes.byref(a), stream_ptr()), "mesm_attn_bwd")


def sine_pos(mask, D):
    """mask (B, L) bool/uint8, True = valid -> (B, L, D) fp32."""
    require_gpu(mask)
    B, L = mask.shape
    m = mask.contiguous()
    out = torch.empty(B, L, D, device=mask.device, dtype=torch.float32)
    check(lib().mesm_sine_pos_fwd(ptr(m), ptr(out), B, L, D, stream_ptr()), "mesm_sine_pos_fwd")
    return out


def query_sine_fwd(ref, D):
    """ref (..., 2) -> (..., D)."""
    require_gpu(ref)
    r2 = ref.reshape(-1, 2).contiguous()
    out = torch.empty(r2.shape[0], D, device=ref.device, dtype=torch.float32)
    check(lib().mesm_query_sine_fwd(ptr(r2), ptr(out), r2.shape[0], D, stream_ptr()),
          "mesm_query_sine_fwd")
    return out.view(*ref.shape[:-1], D)


def query_sine_bwd(ref, dout):
    require_gpu(ref, dout)
    D = dout.shape[-1]
    r2 = ref.reshape(-1, 2).contiguous()
    d2 = dout.reshape(-1, D).contiguous()
    dref = zeros(r2.shape, r2.device)
    check(lib().mesm_query_sine_bwd(ptr(r2), ptr(d2), ptr(dref), r2.shape[0], D, stream_ptr()),
          "mesm_query_sine_bwd")
    return dref.view(ref.shape)


def _check_drop_index(numel, p):
    """every dropout site hashes a 32-bit element index: refuse tensors it would wrap on"""
    if p > 0.0 and numel >= (1 << 32):
        raise _lib.MesmError("dropout over %d elements: the counter-hash index is 32-bit" % numel)


def dropout(x, p, seed, out=None):
    require_gpu(x)
    assert x.is_contiguous()
    _check_drop_index(x.numel(), p)
    y = torch.empty_like(x) if out is None else out
    check(lib().mesm_dropout(ptr(x), ptr(y), x.numel(), float(p), int(seed) & 0xFFFFFFFF,
                             ptr(_seed_offset), stream_ptr()), "mesm_dropout")
    return y


def act_dropout(x, act, slope, p, seed):
    """dropout(act(x)) with the library's counter-based mask (flat element index)."""
    require_gpu(x)
    assert x.is_contiguous()
    y = torch.empty_like(x)
    check(lib().mesm_act_dropout(ptr(x), ptr(y), x.numel(), int(act), ptr(slope), float(p),
                                 int(seed) & 0xFFFFFFFF, ptr(_seed_offset), stream_ptr()), "mesm_act_dropout")
    return y


def act_bias_bwd(dy, ref, act, dbias=None, slope=None, dslope=None, inplace=False):
    """dz = dy * act'(ref); dbias += colsum(dz); returns dz (dy itself if inplace)."""
    require_gpu(dy)
    cols = dy.shape[-1]
    dy2 = dy.reshape(-1, cols)
    assert dy2.is_contiguous()
    ref2 = ref.reshape(-1, cols) if ref is not None else None
    if act == ACT_NONE:
        dz = None
    else:
        dz = dy2 if inplace else torch.empty_like(dy2)
    check(lib().mesm_act_bias_bwd(ptr(dy2), ptr(ref2), ptr(dz), ptr(dbias), ptr(slope),
                                  ptr(dslope), dy2.shape[0], cols, act, stream_ptr()),
          "mesm_act_bias_bwd")
    return (dz if dz is not None else dy2).view(dy.shape)


# ----------------------------------------------------------------------------- losses
def nll_smooth_fwd(logit, label, mask, eps=0.1):
    """logit (R, C), label (R,) int64, mask (R,) bool -> row_loss (R), row_lse (R), correct (R) uint8."""
    require_gpu(logit, label, mask)
    R, C = logit.shape
    assert logit.is_contiguous() and label.dtype == torch.int64 and label.is_contiguous()
    m = mask.contiguous() if mask is not None else None
    row_loss = torch.empty(R, device=logit.device, dtype=torch.float32)
    row_lse = torch.empty(R, device=logit.device, dtype=torch.float32)
    correct = torch.empty(R, device=logit.device, dtype=torch.uint8)
    check(lib().mesm_nll_smooth_fwd(ptr(logit), ptr(label), ptr(m), ptr(row_loss), ptr(row_lse),
                                    ptr(correct), R, C, float(eps), stream_ptr()),
          "mesm_nll_smooth_fwd")
    return row_loss, row_lse, correct


def nll_smooth_bwd(logit, label, row_lse, row_grad, eps=0.1):
    require_gpu(logit, label, row_lse, row_grad)
    R, C = logit.shape
    dlogit = torch.empty_like(logit)
    check(lib().mesm_nll_smooth_bwd(ptr(logit), ptr(label), ptr(row_lse), ptr(row_grad.contiguous()),
                                    ptr(dlogit), R, C, float(eps), stream_ptr()),
          "mesm_nll_smooth_bwd")
    return dlogit


def saliency_loss_fwd(s_pos, s_neg, label64, vmask, pos_idx, neg_idx, rank_coef, margin, out=None, n_valid=None):
    require_gpu(s_pos, s_neg, label64, vmask)
    N, L = s_pos.shape
    assert label64.dtype == torch.float64 and label64.is_contiguous()
    assert s_pos.is_contiguous() and s_neg.is_contiguous() and vmask.is_contiguous()
    P = pos_idx.shape[1] if pos_idx is not None else 0
    if out is None:
        out = torch.empty(1, device=s_pos.device, dtype=torch.float32)
    check(lib().mesm_saliency_loss_fwd_nv(ptr(s_pos), ptr(s_neg), ptr(label64), ptr(vmask),
                                          ptr(pos_idx), ptr(neg_idx), N, L, P, float(rank_coef),
                                          float(margin), ptr(out), ptr(n_valid), stream_ptr()),
          "mesm_saliency_loss_fwd")
    return out


def saliency_loss_bwd(s_pos, s_neg, label64, vmask, pos_idx, neg_idx, rank_coef, margin, gscale, out=None, n_valid=None):
    """out: (ds_pos, ds_neg) to write into (e.g. the two halves of one stacked gradient)"""
    N, L = s_pos.shape
    P = pos_idx.shape[1] if pos_idx is not None else 0
    ds_pos, ds_neg = out if out is not None else (torch.empty_like(s_pos), torch.empty_like(s_neg))
    assert ds_pos.is_contiguous() and ds_neg.is_contiguous()
    check(lib().mesm_saliency_loss_bwd_nv(ptr(s_pos), ptr(s_neg), ptr(label64), ptr(vmask),
                                          ptr(pos_idx), ptr(neg_idx), N, L, P, float(rank_coef),
                                          float(margin), ptr(gscale), ptr(ds_pos), ptr(ds_neg), ptr(n_valid),
                                          stream_ptr()), "mesm_saliency_loss_bwd")
    return ds_pos, ds_neg


def _check_match_limits(Q, Tmax):
    """The in-kernel assignment keeps its fp64 work arrays in LDS (60 KB per workgroup) and the matched set in a
    64-bit mask: say so here instead of returning an opaque status code.  Any (Q x T) shape within these extents
    is solved like the reference's scipy call (matcher.py:108-117), T > Q included."""
    if Q > 64 or Tmax > 64:
        raise _lib.MesmError(
            "Hungarian matching kernel: num_queries = %d, target windows per pair = %d (limit 64 each); the "
            "shipped configs use 10 queries and <= 5 windows (qvhighlights.py:148-150)" % (Q, Tmax))


def match(logits, spans, tgt_cxw, tgt_xx, tgt_off, Tmax, w_span, w_giou, w_class, want_cost=False):
    """logits (N,Q,2), spans (N,Q,2), targets (sumT,2) x2, tgt_off (N+1) int32 ->
    match_q (sumT) int32 (-1 = target left unmatched, only where a pair has more targets than queries)
    [, cost (N,Q,Tmax)]."""
    require_gpu(logits, spans, tgt_cxw, tgt_xx, tgt_off)
    N, Q, _ = logits.shape
    assert tgt_off.dtype == torch.int32
    _check_match_limits(Q, Tmax)
    match_q = torch.empty(tgt_cxw.shape[0], device=logits.device, dtype=torch.int32)
    cost = torch.zeros(N, Q, Tmax, device=logits.device, dtype=torch.float32) if want_cost else None
    check(lib().mesm_match(ptr(logits.contiguous()), ptr(spans.contiguous()), ptr(tgt_cxw.contiguous()),
                           ptr(tgt_xx.contiguous()), ptr(tgt_off), N, Q, int(Tmax), float(w_span),
                           float(w_giou), float(w_class), ptr(cost), ptr(match_q), stream_ptr()),
          "mesm_match")
    return (match_q, cost) if want_cost else match_q


# ----------------------------------------------------------------------------- fused criterion
def set_loss_fwd(logits, spans, tgt_cxw, tgt_xx, tgt_off, Tmax, w_span, w_giou, w_class, eos_coef, out4, n_valid=None):
    """Match + span/gIoU/label losses of one decoder layer; writes out4 (4 floats), returns match_q."""
    require_gpu(logits, spans, tgt_cxw, tgt_xx, tgt_off, out4)
    N, Q, _ = logits.shape
    assert logits.is_contiguous() and spans.is_contiguous() and tgt_off.dtype == torch.int32
    _check_match_limits(Q, Tmax)
    match_q = torch.empty(tgt_cxw.shape[0], device=logits.device, dtype=torch.int32)
    check(lib().mesm_set_loss_fwd_nv(ptr(logits), ptr(spans), ptr(tgt_cxw), ptr(tgt_xx), ptr(tgt_off), N, Q,
                                     int(Tmax), float(w_span), float(w_giou), float(w_class),
                                     float(eos_coef), ptr(match_q), ptr(out4), ptr(n_valid), stream_ptr()),
          "mesm_set_loss_fwd")
    return match_q


def set_loss_fwd_layers(layers, tgt_cxw, tgt_xx, tgt_off, Tmax, w_span, w_giou, w_class, eos_coef, n_valid=None):
    """layers: [(logits, spans, out4), ...] of the decoder layers (main + auxiliary): one launch, a workgroup per
    layer; -> [match_q, ...]."""
    n = len(layers)
    N, Q, _ = layers[0][0].shape
    _check_match_limits(Q, Tmax)
    mqs = [torch.empty(tgt_cxw.shape[0], device=layers[0][0].device, dtype=torch.int32) for _ in range(n)]
    for lg, sp, o4 in layers:
        require_gpu(lg, sp, o4)
        assert lg.is_contiguous() and sp.is_contiguous() and lg.shape == (N, Q, 2)
    P = ctypes.c_void_p * n
    check(lib().mesm_set_loss_fwd_layers(P(*[t[0].data_ptr() for t in layers]), P(*[t[1].data_ptr() for t in layers]), n,
                                         ptr(tgt_cxw), ptr(tgt_xx), ptr(tgt_off), N, Q, int(Tmax), float(w_span),
                                         float(w_giou), float(w_class), float(eos_coef),
                                         P(*[m.data_ptr() for m in mqs]), P(*[t[2].data_ptr() for t in layers]),
                                         ptr(n_valid), stream_ptr()), "mesm_set_loss_fwd_layers")
    return mqs


def set_loss_bwd(logits, spans, tgt_cxw, tgt_xx, tgt_off, match_q, eos_coef, g3, out=None, n_valid=None):
    """out: (dlogits, dspans) to write into (e.g. one layer's slice of the stacked decoder outputs' gradient)"""
    N, Q, _ = logits.shape
    dlogits, dspans = out if out is not None else (torch.empty_like(logits), torch.empty_like(spans))
    assert dlogits.is_contiguous() and dspans.is_contiguous()
    check(lib().mesm_set_loss_bwd_nv(ptr(logits), ptr(spans), ptr(tgt_cxw), ptr(tgt_xx), ptr(tgt_off),
                                     ptr(match_q), N, Q, float(eos_coef), ptr(g3), ptr(dlogits),
                                     ptr(dspans), ptr(n_valid), stream_ptr()), "mesm_set_loss_bwd")
    return dlogits, dspans


def rec_ss_fwd(pv, cmask, ew, wmask, pos, tau, out, n_valid=None):
    """-> saved (cn, wn, stats, sim); writes the loss into out (1 float)."""
    require_gpu(pv, cmask, ew, wmask, pos, out)
    N, Lv, D = pv.shape
    Le = ew.shape[1]
    assert pv.is_contiguous() and ew.is_contiguous() and cmask.is_contiguous() and wmask.is_contiguous()
    assert pos.shape == (N, N) and pos.is_contiguous()
    dev = pv.device
    cn = torch.empty(N, D, device=dev, dtype=torch.float32)
    wn = torch.empty(N, D, device=dev, dtype=torch.float32)
    stats = torch.empty(2 * N, 4, device=dev, dtype=torch.float32)  # rows N.. : per-row loss staging
    sim = torch.empty(N, N, device=dev, dtype=torch.float32)
    check(lib().mesm_rec_ss_fwd_nv(ptr(pv), ptr(cmask), Lv, ptr(ew), ptr(wmask), Le, ptr(pos), N, D,
                                   float(tau), ptr(cn), ptr(wn), ptr(stats), ptr(sim), ptr(out), ptr(n_valid),
                                   stream_ptr()), "mesm_rec_ss_fwd")
    return cn, wn, stats, sim


def rec_ss_bwd(saved, pos, cmask, wmask, Lv, Le, tau, g, n_valid=None):
    cn, wn, stats, sim = saved
    N, D = cn.shape
    dpv = torch.empty(N, Lv, D, device=cn.device, dtype=torch.float32)
    dew = torch.empty(N, Le, D, device=cn.device, dtype=torch.float32)
    check(lib().mesm_rec_ss_bwd_nv(ptr(cn), ptr(wn), ptr(pos), ptr(sim), ptr(stats), ptr(cmask), ptr(wmask),
                                   N, D, Lv, Le, float(tau), ptr(g), ptr(dpv), ptr(dew), ptr(n_valid), stream_ptr()),
          "mesm_rec_ss_bwd")
    return dpv, dew


def rec_fw_reduce(row_loss, correct, mask, out2, n_valid=None):
    N, Lw = mask.shape
    check(lib().mesm_rec_fw_reduce_nv(ptr(row_loss), ptr(correct), ptr(mask), N, Lw, ptr(out2), ptr(n_valid),
                                      stream_ptr()), "mesm_rec_fw_reduce")


def rec_fw_rowgrad(mask, g, n_valid=None):
    N, Lw = mask.shape
    rg = torch.empty(N * Lw, device=mask.device, dtype=torch.float32)
    check(lib().mesm_rec_fw_rowgrad_nv(ptr(mask), N, Lw, ptr(g), ptr(rg), ptr(n_valid), stream_ptr()),
          "mesm_rec_fw_rowgrad")
    return rg


def rowdot_fwd(a, b, scale):
    """a (N, L, D), b (N, D) -> (N, L): <a[n,l], b[n]> * scale."""
    require_gpu(a, b)
    N, L, D = a.shape
    assert a.is_contiguous() and b.is_contiguous() and b.shape == (N, D)
    s = torch.empty(N, L, device=a.device, dtype=torch.float32)
    check(lib().mesm_rowdot_fwd(ptr(a), ptr(b), N, L, D, float(scale), ptr(s), stream_ptr()),
          "mesm_rowdot_fwd")
    return s


def rowdot_bwd(a, b, ds, scale):
    N, L, D = a.shape
    da = torch.empty_like(a)
    db = torch.empty_like(b)
    check(lib().mesm_rowdot_bwd(ptr(a), ptr(b), ptr(ds), N, L, D, float(scale), ptr(da), ptr(db),
                                stream_ptr()), "mesm_rowdot_bwd")
    return da, db


def text_prep(x, normalize=True):
    """post_process_text: (N, Lw, D) word features -> words, words_mask (bool), sentence feature."""
    require_gpu(x)
    x = x.contiguous()
    N, Lw, D = x.shape
    words = torch.empty_like(x)
    wmask = torch.empty(N, Lw, device=x.device, dtype=torch.bool)
    sent = torch.empty(N, D, device=x.device, dtype=torch.float32)
    check(lib().mesm_text_prep(ptr(x), N, Lw, D, 1 if normalize else 0, ptr(words), ptr(wmask), ptr(sent),
                               stream_ptr()), "mesm_text_prep")
    return words, wmask, sent


def weighted_sum(vals, weights):
    require_gpu(vals, weights)
    out = torch.empty((), device=vals.device, dtype=torch.float32)
    check(lib().mesm_weighted_sum(ptr(vals), ptr(weights), vals.numel(), ptr(out), stream_ptr()),
          "mesm_weighted_sum")
    return out


def scale_vec(g, weights):
    out = torch.empty_like(weights)
    check(lib().mesm_scale_vec(ptr(g), ptr(weights), weights.numel(), ptr(out), stream_ptr()),
          "mesm_scale_vec")
    return out


def criterion_fwd(lv, weights, N, n_valid=None, set_losses=None, sal=None, recfw=None, recss=None):
    """The criterion's forward in three launches (mesm_criterion_fwd): every block's first stage in one grid, rec_ss'
    similarity rows, one finishing workgroup.  Writes the blocks' values into their slots of `lv`; -> (total, saved) with
    saved = dict(match=[...], row_lse=..., recss=(cn, wn, stats, sim)) for the backward.
    set_losses: dict(Q, Tmax, w_span, w_giou, w_class, eos_coef, tgt_cxw, tgt_xx, tgt_off, layers=[(logits, spans, slot)]);
    sal: dict(s_pos, s_neg, label, vmask, pos_idx, neg_idx, rank_coef, margin, slot);
    recfw: dict(logit (N, Lw, C), label, mask (N, Lw), eps, slot);  recss: dict(pv, cmask, ew, wmask, pos, tau, slot)."""
    require_gpu(lv, weights)
    dev = lv.device
    a = _lib.CritFwdArgs()
    total = torch.empty((), device=dev, dtype=torch.float32)
    a.weights, a.lv, a.total, a.n_valid, a.N, a.n_slots = ptr(weights), ptr(lv), ptr(total), ptr(n_valid), N, lv.numel()
    saved = {}
    if set_losses:
        lay = set_losses["layers"]
        assert 0 < len(lay) <= 8
        _check_match_limits(set_losses["Q"], set_losses["Tmax"])
        a.Q, a.Tmax, a.n_set = set_losses["Q"], set_losses["Tmax"], len(lay)
        a.w_span, a.w_giou, a.w_class = float(set_losses["w_span"]), float(set_losses["w_giou"]), float(set_losses["w_class"])
        a.eos_coef = float(set_losses["eos_coef"])
        a.tgt_cxw, a.tgt_xx, a.tgt_off = ptr(set_losses["tgt_cxw"]), ptr(set_losses["tgt_xx"]), ptr(set_losses["tgt_off"])
        sumT = set_losses["tgt_cxw"].shape[0]
        mqs = torch.empty(len(lay), max(sumT, 1), dtype=torch.int32, device=dev)
        saved["match"] = [mqs[l, :sumT] for l in range(len(lay))]
        for l, (lg, sp, slot) in enumerate(lay):
            assert lg.is_contiguous() and sp.is_contiguous()
            a.set_logits[l], a.set_spans[l], a.set_match[l], a.set_slot[l] = ptr(lg), ptr(sp), ptr(mqs[l]), slot
    if sal:
        _, L = sal["s_pos"].shape
        assert sal["label"].dtype == torch.float64 and sal["label"].is_contiguous()
        assert sal["s_pos"].is_contiguous() and sal["s_neg"].is_contiguous() and sal["vmask"].is_contiguous()
        a.sal_on, a.sal_L, a.sal_slot = 1, L, sal["slot"]
        a.sal_P = sal["pos_idx"].shape[1] if sal["pos_idx"] is not None else 0
        a.rank_coef, a.margin = float(sal["rank_coef"]), float(sal["margin"])
        a.s_pos, a.s_neg, a.sal_label, a.vmask = ptr(sal["s_pos"]), ptr(sal["s_neg"]), ptr(sal["label"]), ptr(sal["vmask"])
        a.pos_idx, a.neg_idx = ptr(sal["pos_idx"]), ptr(sal["neg_idx"])
    if recfw:
        N_, Lw, C = recfw["logit"].shape
        assert recfw["logit"].is_contiguous()
        R = N_ * Lw
        row_loss = torch.empty(R, device=dev, dtype=torch.float32)
        row_lse = torch.empty(R, device=dev, dtype=torch.float32)
        correct = torch.empty(R, device=dev, dtype=torch.uint8)
        a.fw_on, a.fw_Lw, a.fw_C, a.fw_slot, a.fw_eps = 1, Lw, C, recfw["slot"], float(recfw["eps"])
        a.logit, a.label, a.words_mask = ptr(recfw["logit"]), ptr(recfw["label"]), ptr(recfw["mask"])
        a.row_loss, a.row_lse, a.correct = ptr(row_loss), ptr(row_lse), ptr(correct)
        saved["row_lse"] = row_lse
        saved["_staging"] = (row_loss, correct)
    if recss:
        pv, ew = recss["pv"], recss["ew"]
        N_, Lv, D = pv.shape
        Le = ew.shape[1]
        assert pv.is_contiguous() and ew.is_contiguous() and recss["cmask"].is_contiguous() and recss["wmask"].is_contiguous()
        assert recss["pos"].shape == (N_, N_) and recss["pos"].is_contiguous()
        cn = torch.empty(N_, D, device=dev, dtype=torch.float32)
        wn = torch.empty(N_, D, device=dev, dtype=torch.float32)
        stats = torch.empty(2 * N_, 4, device=dev, dtype=torch.float32)  # rows N.. : per-row loss staging
        sim = torch.empty(N_, N_, device=dev, dtype=torch.float32)
        a.ss_on, a.ss_D, a.ss_Lv, a.ss_Le, a.ss_slot, a.ss_tau = 1, D, Lv, Le, recss["slot"], float(recss["tau"])
        a.pv, a.cmask, a.ew, a.wmask, a.ss_pos = ptr(pv), ptr(recss["cmask"]), ptr(ew), ptr(recss["wmask"]), ptr(recss["pos"])
        a.cn, a.wn, a.stats, a.sim = ptr(cn), ptr(wn), ptr(stats), ptr(sim)
        saved["recss"] = (cn, wn, stats, sim)
    check(lib().mesm_criterion_fwd(ctypes.byref(a), stream_ptr()), "mesm_criterion_fwd")
    return total, saved


def criterion_bwd(g_total, weights, N, n_valid=None, set_losses=None, sal=None, recfw=None, recss=None):
    """The criterion's whole backward as one launch (mesm_criterion_bwd): each block multiplies d total by its own weight.
    set_losses: dict(Q, eos_coef, tgt_cxw, tgt_xx, tgt_off, layers=[(logits, spans, match_q, dlogits, dspans, slot)]);
    sal: dict(s_pos, s_neg, label, vmask, pos_idx, neg_idx, rank_coef, margin, ds_pos, ds_neg, slot);
    recfw: dict(logit (N, Lw, C), label, row_lse, mask (N, Lw), eps, dlogit, slot);
    recss: dict(saved=(cn, wn, stats, sim), pos, cmask, wmask, Lv, Le, tau, dpv, dew, slot)."""
    require_gpu(g_total, weights)
    a = _lib.CritBwdArgs()
    a.g_total, a.weights, a.n_valid, a.N = ptr(g_total), ptr(weights), ptr(n_valid), N
    keep = []
    if set_losses:
        lay = set_losses["layers"]
        assert 0 < len(lay) <= 8
        a.Q, a.n_set, a.eos_coef = set_losses["Q"], len(lay), float(set_losses["eos_coef"])
        a.tgt_cxw, a.tgt_xx, a.tgt_off = ptr(set_losses["tgt_cxw"]), ptr(set_losses["tgt_xx"]), ptr(set_losses["tgt_off"])
        for l, (lg, sp, mq, dl, dsp, slot) in enumerate(lay):
            assert lg.is_contiguous() and sp.is_contiguous() and dl.is_contiguous() and dsp.is_contiguous()
            a.set_logits[l], a.set_spans[l], a.set_match[l] = ptr(lg), ptr(sp), ptr(mq)
            a.set_dlogits[l], a.set_dspans[l], a.set_slot[l] = ptr(dl), ptr(dsp), slot
    if sal:
        N_, L = sal["s_pos"].shape
        assert sal["ds_pos"].is_contiguous() and sal["ds_neg"].is_contiguous()
        a.sal_on, a.sal_L, a.sal_slot = 1, L, sal["slot"]
        a.sal_P = sal["pos_idx"].shape[1] if sal["pos_idx"] is not None else 0
        a.rank_coef, a.margin = float(sal["rank_coef"]), float(sal["margin"])
        a.s_pos, a.s_neg, a.sal_label, a.vmask = ptr(sal["s_pos"]), ptr(sal["s_neg"]), ptr(sal["label"]), ptr(sal["vmask"])
        a.pos_idx, a.neg_idx, a.ds_pos, a.ds_neg = ptr(sal["pos_idx"]), ptr(sal["neg_idx"]), ptr(sal["ds_pos"]), ptr(sal["ds_neg"])
    if recfw:
        _, Lw, C = recfw["logit"].shape
        a.fw_on, a.fw_Lw, a.fw_C, a.fw_slot, a.fw_eps = 1, Lw, C, recfw["slot"], float(recfw["eps"])
        a.logit, a.label, a.row_lse = ptr(recfw["logit"]), ptr(recfw["label"]), ptr(recfw["row_lse"])
        a.words_mask, a.dlogit = ptr(recfw["mask"]), ptr(recfw["dlogit"])
    if recss:
        cn, wn, stats, sim = recss["saved"]
        a.ss_on, a.ss_D, a.ss_Lv, a.ss_Le, a.ss_slot = 1, cn.shape[1], recss["Lv"], recss["Le"], recss["slot"]
        a.ss_tau = float(recss["tau"])
        a.cn, a.wn, a.ss_pos, a.sim, a.stats = ptr(cn), ptr(wn), ptr(recss["pos"]), ptr(sim), ptr(stats)
        a.cmask, a.wmask, a.dpv, a.dew = ptr(recss["cmask"]), ptr(recss["wmask"]), ptr(recss["dpv"]), ptr(recss["dew"])
    check(lib().mesm_criterion_bwd(ctypes.byref(a), stream_ptr()), "mesm_criterion_bwd")


# ----------------------------------------------------------------------------- assembly kernels (csrc/glue.hip)
def _u8(t):
    return t if t.dtype == torch.uint8 else t.view(torch.uint8)


_glue_defer = 0


class glue_deferred:
    """Inside an open launch phase, the assembly kernels called in this block are QUEUED for the phase's one grouped
    launch (mesm_glue_group) instead of running at once -- for callers whose assembly calls are independent of everything
    else in the phase (ops.glue_block).  Without it an assembly kernel called inside a phase runs immediately, i.e. before
    the phase's queued launches (what the transformer blocks rely on)."""

    def __enter__(self):
        global _glue_defer
        _glue_defer += 1

    def __exit__(self, *a):
        global _glue_defer
        _glue_defer -= 1
        return False


def glue_deferring():
    return _phase is not None and _glue_defer > 0


def _glue(op, p, n=(), i=(), keep=()):
    """one assembly problem: queued in the open phase (glue_deferred) or launched on its own through the grouped entry"""
    a = _lib.GlueArgs()
    a.op = op
    for k, t in enumerate(p):
        a.p[k] = t.data_ptr() if torch.is_tensor(t) else t
    for k, v in enumerate(n):
        a.n[k] = int(v)
    for k, v in enumerate(i):
        a.i[k] = int(v)
    if glue_deferring():
        _phase.add("glue", a, tuple(keep))
    else:
        check(lib().mesm_glue_group(ctypes.byref(a), 1, stream_ptr()), "mesm_glue_group")


def stack_rows(tensors, gather, idx):
    """[t ; t[idx]] (gather flag 1) or [t ; t] (0) along dim 0 for up to 8 tensors of N rows, one launch."""
    require_gpu(*tensors)
    n, N = len(tensors), tensors[0].shape[0]
    srcs = [t.contiguous() for t in tensors]
    outs = [torch.empty((2 * N,) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype) for t in srcs]
    rb = [t[0].numel() * t.element_size() for t in srcs]
    arr_s = (ctypes.c_void_p * n)(*[t.data_ptr() for t in srcs])
    arr_d = (ctypes.c_void_p * n)(*[t.data_ptr() for t in outs])
    arr_b = (ctypes.c_int64 * n)(*rb)
    arr_g = (ctypes.c_int32 * n)(*[int(g) for g in gather])
    assert all(t.shape[0] == N for t in srcs) and (idx is None or (idx.dtype == torch.int64 and idx.numel() == N))
    if glue_deferring():
        for t, o, b, g in zip(srcs, outs, rb, gather):
            _glue(_lib.GLUE_STACK_ROWS, (t, o, idx if g else None), n=(b,), i=(N,), keep=(t, o, idx))
        return outs
    check(lib().mesm_stack_rows(arr_s, arr_d, arr_b, arr_g, n, ptr(idx), N, stream_ptr()), "mesm_stack_rows")
    return outs


def unstack_rows(d2, idx, N):
    require_gpu(d2)
    d2 = d2.contiguous()
    R = d2[0].numel()
    dx = torch.empty((N,) + tuple(d2.shape[1:]), device=d2.device, dtype=torch.float32)
    if glue_deferring():
        _glue(_lib.GLUE_UNSTACK_ROWS, (d2, idx, dx), n=(R,), i=(N,), keep=(d2, idx, dx))
        return dx
    check(lib().mesm_unstack_rows(ptr(d2), ptr(idx), ptr(dx), N, R, stream_ptr()), "mesm_unstack_rows")
    return dx


def prepend_fwd(tok, x, ptok=None, pos=None, pad=None, first_pad=True):
    """-> xo (B, L+1, D) [, po, xp] [, pado]; tok (D,) shared or (B, D) per row."""
    require_gpu(tok, x)
    B, L, D = x.shape
    assert x.is_contiguous() and tok.is_contiguous() and tok.numel() in (D, B * D)
    per_row = 1 if (tok.numel() == B * D and tok.dim() == 2) else 0
    xo = torch.empty(B, L + 1, D, device=x.device, dtype=torch.float32)
    po = xp = pado = None
    if ptok is not None:
        assert pos.is_contiguous() and pos.shape == x.shape and ptok.numel() == D
        po, xp = torch.empty_like(xo), torch.empty_like(xo)
    if pad is not None:
        assert pad.is_contiguous() and pad.shape == (B, L)
        pado = torch.empty(B, L + 1, device=x.device, dtype=pad.dtype)
    check(lib().mesm_prepend_fwd(ptr(tok), ptr(x), ptr(ptok), ptr(pos), ptr(pad), ptr(xo), ptr(po), ptr(xp),
                                 ptr(pado), B, L, D, per_row, 1 if first_pad else 0, stream_ptr()), "mesm_prepend_fwd")
    return xo, po, xp, pado


def prepend_bwd(dxo, dxp, dpo, dx, dtok, dptok, B, L, D, per_row):
    check(lib().mesm_prepend_bwd(ptr(dxo), ptr(dxp), ptr(dpo), ptr(dx), ptr(dtok), ptr(dptok), B, L, D,
                                 1 if per_row else 0, stream_ptr()), "mesm_prepend_bwd")


def split_token_fwd(mem, Bd):
    require_gpu(mem)
    B, S, D = mem.shape
    assert mem.is_contiguous()
    g = torch.empty(B, D, device=mem.device, dtype=torch.float32)
    loc = torch.empty(B, S - 1, D, device=mem.device, dtype=torch.float32)
    dec = torch.empty(Bd, S - 1, D, device=mem.device, dtype=torch.float32) if Bd else None
    check(lib().mesm_split_token_fwd(ptr(mem), ptr(g), ptr(loc), ptr(dec), B, S - 1, D, Bd, stream_ptr()),
          "mesm_split_token_fwd")
    return g, loc, dec


def split_token_bwd(dg, dloc, ddec, B, L, D, Bd, device):
    dmem = torch.empty(B, L + 1, D, device=device, dtype=torch.float32)
    check(lib().mesm_split_token_bwd(ptr(dg), ptr(dloc), ptr(ddec), ptr(dmem), B, L, D, Bd, stream_ptr()),
          "mesm_split_token_bwd")
    return dmem


def token_mix_fwd(x, m1, tok1, m2=None, tok2=None):
    require_gpu(x, m1, tok1)
    D = x.shape[-1]
    assert x.is_contiguous() and m1.is_contiguous() and m1.numel() * D == x.numel()
    y = torch.empty_like(x)
    if glue_deferring():
        _glue(_lib.GLUE_TOKEN_MIX_FWD, (x, m1, tok1, m2, tok2, y), n=(m1.numel(),), i=(D,), keep=(x, m1, tok1, m2, tok2, y))
        return y
    check(lib().mesm_token_mix_fwd(ptr(x), ptr(m1), ptr(tok1), ptr(m2), ptr(tok2), ptr(y), m1.numel(), D, stream_ptr()),
          "mesm_token_mix_fwd")
    return y


def token_mix_bwd(dy, m1, m2, dx, dtok1, dtok2):
    D = dy.shape[-1]
    if glue_deferring():
        _glue(_lib.GLUE_TOKEN_MIX_BWD, (dy, m1, m2, dx, dtok1, dtok2), n=(m1.numel(),), i=(D,), keep=(dy, m1, m2, dx, dtok1, dtok2))
        return
    check(lib().mesm_token_mix_bwd(ptr(dy), ptr(m1), ptr(m2), ptr(dx), ptr(dtok1), ptr(dtok2), m1.numel(), D,
                                   stream_ptr()), "mesm_token_mix_bwd")


def gather_rows_fwd(x2d, idx, valid=None, normalize=False):
    """y[j] = valid[j] ? x2d[idx[j]] : 0 (optionally L2-normalised) -> y (*idx.shape, D), rnorm or None."""
    require_gpu(x2d, idx)
    assert x2d.dim() == 2 and x2d.is_contiguous() and idx.dtype == torch.int64 and idx.is_contiguous()
    D = x2d.shape[1]
    y = torch.empty(*idx.shape, D, device=x2d.device, dtype=torch.float32)
    rn = torch.empty(idx.numel(), device=x2d.device, dtype=torch.float32) if normalize else None
    if glue_deferring():
        _glue(_lib.GLUE_GATHER_ROWS_FWD, (x2d, idx, valid, y, rn), n=(idx.numel(),), i=(D, 1 if normalize else 0),
              keep=(x2d, idx, valid, y, rn))
        return y, rn
    check(lib().mesm_gather_rows_fwd(ptr(x2d), ptr(idx), ptr(valid), ptr(y), ptr(rn), idx.numel(), D,
                                     1 if normalize else 0, stream_ptr()), "mesm_gather_rows_fwd")
    return y, rn


def gather_rows_bwd(dy, y, rnorm, inv, valid, src_rows, normalize):
    D = dy.shape[-1]
    dx = torch.empty(src_rows, D, device=dy.device, dtype=torch.float32)
    if glue_deferring():
        _glue(_lib.GLUE_GATHER_ROWS_BWD, (dy, y, rnorm, inv, valid, dx), n=(src_rows,), i=(D, 1 if normalize else 0),
              keep=(dy, y, rnorm, inv, valid, dx))
        return dx
    check(lib().mesm_gather_rows_bwd(ptr(dy), ptr(y), ptr(rnorm), ptr(inv), ptr(valid), ptr(dx), src_rows, D,
                                     1 if normalize else 0, stream_ptr()), "mesm_gather_rows_bwd")
    return dx


def step_begin(ring, slot_bytes, slots, dst, pull_ctr, seed_ctr=None):
    """first node of a captured step: dst <- ring[*pull_ctr % slots] (ring: PINNED host uint8 tensor), counters += 1"""
    require_gpu(dst, pull_ctr)
    assert ring.is_pinned() and ring.numel() >= slot_bytes * slots and dst.numel() * dst.element_size() >= slot_bytes
    check(lib().mesm_step_begin(ring.data_ptr(), int(slot_bytes), int(slots), ptr(dst), ptr(pull_ctr),
                                ptr(seed_ctr) if seed_ctr is not None else None, stream_ptr()), "mesm_step_begin")


def add_n(ts):
    """sum of 1-8 contiguous fp32 tensors of one shape, one launch"""
    require_gpu(*ts)
    assert 1 <= len(ts) <= 8 and all(t.is_contiguous() and t.shape == ts[0].shape and t.dtype == torch.float32 for t in ts)
    out = torch.empty_like(ts[0])
    arr = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    check(lib().mesm_add_n(arr, len(ts), ptr(out), out.numel(), stream_ptr()), "mesm_add_n")
    return out


def add_tile(a, b, reps):
    """[a + b] repeated `reps` times along dim 0 (a, b of one shape): the stacked passes' video + position sum formed
    from the unstacked tensors (model.py:175-180, 281-286), one member of a grouped assembly launch."""
    require_gpu(a, b)
    assert a.is_contiguous() and b.is_contiguous() and a.shape == b.shape and a.dtype == torch.float32
    out = torch.empty((reps * a.shape[0],) + tuple(a.shape[1:]), device=a.device, dtype=torch.float32)
    nb = (ctypes.c_int64 * 1)(b.numel())
    i2 = (ctypes.c_int32 * 2).from_buffer(nb)
    _glue(_lib.GLUE_ADD_TILE, (a, b, out), n=(out.numel(), a.numel()), i=(i2[0], i2[1]), keep=(a, b, out))
    return out


def gather_add(a2d, b2d, idx, valid=None):
    """y[j] = valid[j] ? a2d[idx[j]] + b2d[idx[j]] : 0 -> (*idx.shape, D): gathered features + their gathered position
    embeddings in one pass (the key-side query of the MLM branch, model.py:312-325 + transformer.py:512)"""
    require_gpu(a2d, b2d, idx)
    assert a2d.dim() == 2 and a2d.shape == b2d.shape and a2d.is_contiguous() and b2d.is_contiguous()
    assert idx.dtype == torch.int64 and idx.is_contiguous()
    D = a2d.shape[1]
    y = torch.empty(*idx.shape, D, device=a2d.device, dtype=torch.float32)
    _glue(_lib.GLUE_GATHER_ADD, (a2d, b2d, idx, valid, y), n=(idx.numel(),), i=(D,), keep=(a2d, b2d, idx, valid, y))
    return y


def add_wrap(a, b):
    """a + b with b repeated along dim 0 (a.numel() a multiple of b.numel())."""
    require_gpu(a, b)
    assert a.is_contiguous() and b.is_contiguous()
    out = torch.empty_like(a)
    check(lib().mesm_add_wrap(ptr(a), ptr(b), ptr(out), a.numel(), b.numel(), stream_ptr()), "mesm_add_wrap")
    return out


SKINNY_OUT = 4  # Linear layers with at most this many output features take skinny_linear_bwd


def skinny_linear_bwd(dz, x, w, dw, db=None, need_dx=True, relu_mask=False):
    """Backward of y = x W^T + b, W (J <= 4, K), in one launch: -> dx (or None); dw += dz^T x, db += colsum(dz)."""
    require_gpu(dz, x, w, dw)
    M, J = dz.shape
    K = x.shape[1]
    assert x.shape[0] == M and tuple(w.shape) == (J, K) and tuple(dw.shape) == (J, K) and 1 <= J <= SKINNY_OUT
    assert dz.is_contiguous() and x.is_contiguous() and w.is_contiguous() and dw.is_contiguous()
    assert db is None or (db.is_contiguous() and db.numel() == J)
    dx = torch.empty_like(x) if need_dx else None
    check(lib().mesm_skinny_linear_bwd(ptr(dz), ptr(x), ptr(w), ptr(dx), ptr(dw), ptr(db), M, K, J,
                                       1 if relu_mask else 0, stream_ptr()), "mesm_skinny_linear_bwd")
    return dx


# ----------------------------------------------------------------------------- frozen text encoders
def clip_embed(ids, tok, pos):
    """ids (N, L) int64, tok (V, D) f32, pos (L, D) f32 -> (N, L, D) fp16."""
    require_gpu(ids, tok, pos)
    N, L = ids.shape
    D = tok.shape[1]
    assert ids.dtype == torch.int64 and tok.dtype == pos.dtype == torch.float32 and pos.shape == (L, D)
    x = torch.empty(N, L, D, device=ids.device, dtype=torch.float16)
    check(lib().mesm_clip_embed(ptr(ids.contiguous()), ptr(tok.contiguous()), ptr(pos.contiguous()), ptr(x), N * L, L,
                                D, tok.shape[0], stream_ptr()), "mesm_clip_embed")
    return x


def layernorm_f16(x, gamma, beta, eps=1e-5):
    require_gpu(x, gamma, beta)
    assert x.dtype == torch.float16 and x.is_contiguous() and gamma.dtype == beta.dtype == torch.float32
    D = x.shape[-1]
    y = torch.empty_like(x)
    check(lib().mesm_layernorm_f16(ptr(x), ptr(gamma), ptr(beta), ptr(y), x.numel() // D, D, float(eps), stream_ptr()),
          "mesm_layernorm_f16")
    return y


def gemm_f16(A, W, bias=None, residual=None, out_f32=False, quick_gelu=False):
    """A (M, K) fp16 or fp32 (rounded to fp16 on load), W (N, K) fp16 -> (M, N) fp16, or the fp16-rounded
    values as fp32 (out_f32)."""
    require_gpu(A, W)
    assert A.dim() == 2 and W.dim() == 2 and A.shape[1] == W.shape[1] and W.dtype == torch.float16
    assert A.stride(1) == 1 and W.stride(1) == 1 and A.dtype in (torch.float16, torch.float32)
    M, K = A.shape
    N = W.shape[0]
    C = torch.empty(M, N, device=A.device, dtype=torch.float32 if out_f32 else torch.float16)
    if bias is not None:
        assert bias.dtype == torch.float16 and bias.numel() == N and bias.is_contiguous()
    if residual is not None:
        assert residual.dtype == torch.float16 and residual.shape == (M, N) and residual.stride(1) == 1
    check(lib().mesm_gemm_f16(ptr(A), 1 if A.dtype == torch.float32 else 0, A.stride(0), ptr(W), W.stride(0), ptr(bias),
                              ptr(residual), residual.stride(0) if residual is not None else 0, ptr(C),
                              1 if out_f32 else 0, C.stride(0), M, N, K, 1 if quick_gelu else 0, stream_ptr()),
          "mesm_gemm_f16")
    return C


def text_pool(x, mask, Lw, normalize=True):
    """x (N, Lx, D) fp16 / fp32, mask (N, Lm) bool -> words (N, Lw, D) f32, sentence (N, D) f32."""
    require_gpu(x, mask)
    assert x.is_contiguous() and x.dtype in (torch.float16, torch.float32)
    N, Lx, D = x.shape
    m = mask.contiguous()
    assert m.dtype in (torch.bool, torch.uint8) and m.shape[0] == N
    words = torch.empty(N, Lw, D, device=x.device, dtype=torch.float32)
    sent = torch.empty(N, D, device=x.device, dtype=torch.float32)
    check(lib().mesm_text_pool(ptr(x), 1 if x.dtype == torch.float16 else 0, ptr(m), N, Lx, m.shape[1], Lw, D,
                               1 if normalize else 0, ptr(words), ptr(sent), stream_ptr()), "mesm_text_pool")
    return words, sent


def text_cache_store(hid, rows, slots, cache, Lw):
    """cache[slots[m], :, :] = hid[rows[m], :Lw, :]: hid (n, Lx, D) fp16, cache (capacity, Lw, D) fp16, rows / slots
    (M,) int32 on the device (clamped to the buffers by the kernel)."""
    require_gpu(hid, rows, slots, cache)
    assert hid.dtype == cache.dtype == torch.float16 and hid.is_contiguous() and cache.is_contiguous()
    assert rows.dtype == slots.dtype == torch.int32 and rows.is_contiguous() and slots.is_contiguous()
    n, Lx, D = hid.shape
    M = rows.numel()
    assert slots.numel() == M and cache.dim() == 3 and tuple(cache.shape[1:]) == (Lw, D) and Lw <= Lx
    if M == 0:
        return
    check(lib().mesm_text_cache_store(ptr(hid), n, Lx, ptr(rows), ptr(slots), M, Lw, D, ptr(cache), cache.shape[0],
                                      stream_ptr()), "mesm_text_cache_store")


def text_pool_slots(cache, slots, mask, normalize=True):
    """text_pool with pair n reading cache[slots[n]]: cache (capacity, Lw, D) fp16, slots (N,) int32, mask (N, Lm >= Lw)
    bool -> words (N, Lw, D) f32, sentence (N, D) f32; the bits of text_pool(cache[slots], mask, Lw, normalize)."""
    require_gpu(cache, slots, mask)
    assert cache.dtype == torch.float16 and cache.is_contiguous() and cache.dim() == 3
    assert slots.dtype == torch.int32 and slots.is_contiguous() and slots.dim() == 1
    capacity, Lw, D = cache.shape
    N = slots.numel()
    m = mask.contiguous()
    assert m.dtype in (torch.bool, torch.uint8) and m.shape[0] == N and m.shape[1] >= Lw
    words = torch.empty(N, Lw, D, device=cache.device, dtype=torch.float32)
    sent = torch.empty(N, D, device=cache.device, dtype=torch.float32)
    check(lib().mesm_text_pool_slots(ptr(cache), capacity, ptr(slots), ptr(m), N, m.shape[1], Lw, D,
                                     1 if normalize else 0, ptr(words), ptr(sent), stream_ptr()), "mesm_text_pool_slots")
    return words, sent


def embed_rows(ids, table):
    require_gpu(ids, table)
    assert ids.dtype == torch.int64 and table.dtype == torch.float32 and table.is_contiguous()
    out = torch.empty(*ids.shape, table.shape[1], device=ids.device, dtype=torch.float32)
    check(lib().mesm_embed_rows(ptr(ids.contiguous()), ptr(table), ptr(out), ids.numel(), table.shape[1],
                                table.shape[0], stream_ptr()), "mesm_embed_rows")
    return out


# ----------------------------------------------------------------------------- instrumentation
def gemm_tape(record):
    check(lib().mesm_gemm_tape(1 if record else 0), "mesm_gemm_tape")


def gemm_tape_replay(reps=1):
    ms, n, fl, by = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
    check(lib().mesm_gemm_tape_replay(stream_ptr(), int(reps), ctypes.byref(ms), ctypes.byref(n),
                                      ctypes.byref(fl), ctypes.byref(by)), "mesm_gemm_tape_replay")
    o, w = ctypes.c_double(), ctypes.c_double()
    check(lib().mesm_gemm_tape_bytes(ctypes.byref(o), ctypes.byref(w)), "mesm_gemm_tape_bytes")
    return {"ms": ms.value, "launches": n.value, "flops": fl.value, "bytes": by.value,
            "bytes_with_sides": w.value * int(reps)}
