"""fp64 reference of the fp16 text-tower kernels (csrc/clip_text.hip) with the fp16 roundings where the header of that
file puts them, and the per-element envelopes of a float32 evaluation the kernels are held to.  Shared by
tests/test_clip_text_kernels_gpu.py (tensors on the device) and tests/test_f16_ref_cpu.py (which pins the placement of
the roundings to oracle/clip_text_oracle.py).  Plain torch, any device; nothing here calls a kernel.

The contract (clip_text.hip, header): fp16 values in memory; every Linear accumulates in fp32 and rounds ONCE to fp16
after the bias; QuickGELU and the residual add round after each fp16 op; LayerNorm runs in fp32 on the widened row and
rounds its output.

Every stage function returns (ref, e): `ref` the fp64 value before the stage's last rounding, `e` >= 0 the envelope of
a legitimate fp32 evaluation of it.  The accepted outputs are the fp16 values in [half(ref - e), half(ref + e)]
(`interval`); `e` is zero where the stage is exact (a sum or a product of two fp16 values is exact in fp32's 24 bits
or, for sums of distant exponents, rounds the same way twice, so one rounding to fp16 is the correctly rounded result).
"""
import math

import torch

U32 = 2.0 ** -24  # unit roundoff of float32

# ---------------------------------------------------------------------------------------------------------- constants
# linear: e = C_LIN * U32 * (|A| |W|^T + |bias|).
# C_LIN_MEASURED is the smallest c (rounded up to two decimals) for which a blocked fp32 accumulation on the CPU in the
# kernel's order (`blocked_f32_linear`: 8 k-values per MFMA, 32 per stage, the fp16 bias added in fp32) stays inside the
# envelope on EVERY case of `LINEAR_SWEEP` below, with and without the bias -- measured against that reference
# evaluation, never against the kernel (tests/test_f16_ref_cpu.py::test_measured_c_of_the_blocked_fp32_linear measures it
# again and fails if it moved).  The largest ratio is 3.3193, at (2464, 512, 2048) unit scale without bias; K = 512 gives
# 1.9-2.9, K <= 96 gives 1.2-2.1.  C_LIN is 4 x that, so another legitimate summation order on the device (the matrix
# core's own order inside its 8 products, a different split of K) does not trip it.  The rigorous worst-case constant
# (~K / 8) would make 38-95 % of the elements ambiguous and is useless as a test.
C_LIN_MEASURED = 3.32
C_LIN = 4.0 * C_LIN_MEASURED  # 13.28

QUICK_GELU_ALPHA = 1.702


def half(x):
    """Round to nearest-even fp16, ONCE.  torch converts fp64 through fp32, which rounds twice (1 + 2^-11 + 2^-30 lands
    on the tie and goes down); so the fp32 intermediate is made round-to-odd first: truncated toward zero with its last
    bit set when inexact, after which the second rounding cannot see a false tie (fp32 has 13 more bits than fp16)."""
    if x.dtype == torch.float16:
        return x
    if x.dtype == torch.float32:
        return x.to(torch.float16)
    f = x.to(torch.float32)
    d = f.double()
    inexact = (d != x) & torch.isfinite(f) & torch.isfinite(x)
    away = inexact & (d.abs() > x.abs())
    f = torch.where(away, torch.nextafter(f, torch.zeros_like(f)), f)
    # an overflow of the fp32 conversion of a finite fp64 stays +-inf: far outside fp16 either way
    bits = f.view(torch.int32)
    bits = torch.where(inexact, bits | 1, bits)
    return bits.view(torch.float32).to(torch.float16)


def next_up(h):
    """the next fp16 value above h (inf and NaN stay)"""
    assert h.dtype == torch.float16
    b = h.view(torch.int16).to(torch.int32) & 0xFFFF
    neg = b >= 0x8000
    nb = torch.where(neg, b - 1, b + 1)
    nb = torch.where(b == 0x8000, torch.ones_like(b), nb)  # -0 -> smallest subnormal
    stay = torch.isnan(h) | (h == float("inf"))
    nb = torch.where(stay, b, nb)
    nb = torch.where(nb >= 0x8000, nb - 0x10000, nb).to(torch.int16)
    return nb.view(torch.float16)


def interval(ref, e):
    """-> (lo, hi) fp16: the accepted outputs are the fp16 values lo <= v <= hi"""
    return half(ref - e), half(ref + e)


def inside(got, ref, e):
    """elementwise: got (fp16, or fp16 values widened) lies in [half(ref - e), half(ref + e)]; a NaN reference accepts
    only NaN"""
    lo, hi = interval(ref, e)
    g = got.double()
    ok = (g >= lo.double()) & (g <= hi.double())
    return ok | (torch.isnan(ref) & torch.isnan(g))


def ambiguous(ref, e):
    """elementwise: the envelope spans more than one fp16 value"""
    lo, hi = interval(ref, e)
    return lo.double() != hi.double()


def candidates(ref, e, limit=4, strict=True):
    """the accepted fp16 values of each element as a list of at most `limit` tensors (repeating the last one where there
    are fewer).  strict: raises if some envelope holds more; otherwise -> (list, wide) with `wide` marking those
    elements (outputs next to zero, where the fp16 values lie closer together than the envelope is wide)."""
    lo, hi = interval(ref, e)
    out = [lo]
    for _ in range(limit - 1):
        nxt = next_up(out[-1])
        out.append(torch.where(nxt.double() <= hi.double(), nxt, out[-1]))
    wide = ~((out[-1].double() >= hi.double()) | torch.isnan(ref))
    if not strict:
        return out, wide
    if bool(wide.any()):
        raise AssertionError("an envelope spans more than %d fp16 values" % limit)
    return out


def same16(a, b):
    """bitwise-equal fp16 values, +0 == -0 and NaN == NaN"""
    return (a == b) | (torch.isnan(a) & torch.isnan(b))


# ------------------------------------------------------------------------------------------------------------- stages
def embed(ids, tok, pos):
    """x[n, l] = fp16(tok[ids[n, l]]) + fp16(pos[l]), one rounding of the exact sum.  ids (N, L) int64 inside the
    table, tok (V, D) and pos (L, D) fp32."""
    v = half(tok)[ids].double() + half(pos).double()
    return v, torch.zeros_like(v)


def layernorm(x16, gamma, beta, eps=1e-5):
    """y = LN(float(x)) * gamma + beta per row of x16 (..., D) fp16; gamma, beta fp32.

    Envelope of an fp32 evaluation, U = 2^-24, kappa = sqrt(D) + 8.  With m the mean, d = x - m, n = d * rstd:
      mean     a sum of D terms and a division.  The kernel's tree (D/64 terms per lane, 6 butterfly levels) has the
               worst-case bound (D/64 + 7) U mean|x| <= kappa U mean|x| for D <= 4096; a sequential sum meets
               sqrt(D) U mean|x| as a random walk.  So |dm| <= kappa U A, A = mean|x| of the row.
      variance sum d^2 / D is stationary in m (sum d = 0), so dm enters at second order only; the rounding of d, of
               the square, the sum of D positive terms, the division and the + eps give a relative kappa U + 4 U.
      rsqrtf   one ulp (2 U) on top of half the variance's error: |drstd| / rstd <= (kappa / 2 + 4) U.
      n        |dn| <= |dm| rstd + |n| ((kappa / 2 + 4) U + 2 U)          (the subtraction, the product)
      y        |dy| <= |gamma| |dn| + U |n gamma| + U |y|                 (the product, the sum)
    which is bounded by  e = U (kappa |gamma| (A rstd + |n|) + |y|).
    A row whose mean is large against its spread has A rstd = |m| / sigma >> 1: the envelope widens there as the
    operation's own conditioning does, and a one-pass variance (relative error ~ U m^2 / sigma^2) still falls outside.
    """
    D = x16.shape[-1]
    x = x16.double()
    m = x.mean(-1, keepdim=True)
    d = x - m
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    n = d * rstd
    g = gamma.double()
    y = n * g + beta.double()
    kappa = math.sqrt(D) + 8.0
    A = x.abs().mean(-1, keepdim=True)
    e = U32 * (kappa * g.abs() * (A * rstd + n.abs()) + y.abs())
    return y, e


def linear(A, W16, bias16=None):
    """A (M, K) fp16, or fp32 (rounded to fp16 first, as load8<float> does while staging); W16 (N, K) fp16; bias16 (N,)
    fp16 or None.  -> (A W^T + bias in fp64, C_LIN U (|A| |W|^T + |bias|))."""
    a = half(A).double()
    w = W16.double()
    ref = a @ w.t()
    mag = a.abs() @ w.abs().t()
    if bias16 is not None:
        ref = ref + bias16.double()
        mag = mag + bias16.double().abs()
    return ref, C_LIN * U32 * mag


def blocked_f32_accumulate(A, W16):
    """A W^T accumulated in fp32 in the kernel's order: per stage of 32 k-values four matrix-core products of 8; the
    fp16 x fp16 products are exact in fp32, the 8 of one product are summed in fp32 in k order and that sum is added
    to the running fp32 accumulator.  Elementwise IEEE operations only (no BLAS), so the result is the same on every
    machine.  -> fp32 (M, N)"""
    a = half(A).float()
    w = W16.float().t().contiguous()  # (K, N)
    K = a.shape[1]
    acc = torch.zeros(a.shape[0], w.shape[1], dtype=torch.float32, device=a.device)
    for k0 in range(0, K, 32):
        for k1 in range(k0, min(k0 + 32, K), 8):
            p = a[:, k1:k1 + 1] * w[k1:k1 + 1]
            for k in range(k1 + 1, min(k1 + 8, K)):
                p.addcmul_(a[:, k:k + 1], w[k:k + 1])
            acc += p
    return acc


def blocked_f32_linear(A, W16, bias16=None, acc=None):
    """`blocked_f32_accumulate` (or a cached result of it, `acc`), then the fp16 bias added in fp32.  -> fp32, BEFORE the
    rounding to fp16.  A reference evaluation: it measures C_LIN and sets the share of elements criterion (b) allows to
    differ from half(ref)."""
    if acc is None:
        acc = blocked_f32_accumulate(A, W16)
    return acc + bias16.float() if bias16 is not None else acc


def quick_gelu_parts(v16):
    """-> (t, sig, es): t = fp16(1.702f * v) (the fp32 product the eager op and the kernel both form, then fp16),
    sig = sigmoid(t) in fp64, es = the ABSOLUTE slack of an fp32 sigmoid 1 / (1 + __expf(-t)):
      __expf(-t) = exp2(-t log2 e): the argument product rounds once (|t log2 e| U) and log2 e itself is off by U / 2
      relative, an absolute 1.5 U |t| log2 e in the exponent = a relative 1.5 U |t| in the result; the hardware exp2 is
      good to one ulp = 2 U.  d sigma / sigma = -(1 - sigma) d(e^-t) / e^-t: the errors of e^-t enter with the factor
      1 - sigma (none at the saturated end sigma -> 1, in full at sigma -> 0).  1 + e^-t rounds once (U) and the division
      once more (U; 5 U if it is the 2.5-ulp approximate one):
          es = sigma ((1 - sigma) (1.5 |t| + 2) + 6) U.
    Where e^-t overflows fp32 (t < -88.7) the kernel gives 0 and sigma < 1e-38 rounds to the fp16 zero as well."""
    t = (v16.float() * QUICK_GELU_ALPHA).to(torch.float16)
    td = t.double()
    sig = torch.sigmoid(td)
    es = sig * (torch.sigmoid(-td) * (1.5 * td.abs().clamp(max=65504.0) + 2.0) + 6.0) * U32  # (t = +-inf: 0 * inf)
    return t, sig, es


def quick_gelu(v16):
    """v * fp16(sigmoid(fp16(1.702 v))), one rounding per fp16 op.  -> (fp64 product before the last rounding, 0): the
    NOMINAL value, with s the correctly rounded sigmoid.  `quick_gelu_accepts` widens s by its slack."""
    _, sig, _ = quick_gelu_parts(v16)
    s = half(sig)
    v = v16.double() * s.double()
    return v, torch.zeros_like(v)


def quick_gelu_candidates(v16, limit=3):
    """every fp16(v * s) with s an accepted fp16 sigmoid of v: a list of fp16 tensors"""
    _, sig, es = quick_gelu_parts(v16)
    ss = candidates(sig, es, limit)  # (a NaN v gives a NaN sigmoid: the product is NaN for every candidate)
    return [half(v16.double() * s.double()) for s in ss]


def add_residual(v16, res16):
    """fp16(v + res): the exact sum, rounded once"""
    v = v16.double() + res16.double()
    return v, torch.zeros_like(v)


def epilogue_accepts(got16, ref, e, gelu=False, res16=None, limit=4):
    """elementwise: got16 is an accepted output of the GEMM epilogue for the accumulator-plus-bias value `ref` with
    envelope `e`: v in [half(ref - e), half(ref + e)], then (gelu) the rounded product of that v with an accepted s, then
    (res16) the rounded exact sum with the residual -- for ANY accepted v and s, by enumeration.
    Where the envelope holds more than `limit` values of v (v next to zero: 2^-24 steps under an envelope of the size of
    the operands) the enumeration gives way to interval arithmetic: t and s are monotone in v, the product v s over
    [lo, hi] x [s_lo, s_hi] is extreme at a corner, and the roundings and the sum with the residual are monotone."""
    vs, wide = candidates(ref, e, limit, strict=False)
    ok = torch.zeros(ref.shape, dtype=torch.bool, device=ref.device)
    for v in vs:
        outs = quick_gelu_candidates(v) if gelu else [v]
        for o in outs:
            if res16 is not None:
                o = half(add_residual(o, res16)[0])
            ok |= same16(got16, o)
    if bool(wide.any()):
        lo, hi = interval(ref, e)
        if gelu:
            _, sig_l, es_l = quick_gelu_parts(lo)
            _, sig_h, es_h = quick_gelu_parts(hi)
            s_lo, s_hi = half(sig_l - es_l).double(), half(sig_h + es_h).double()
            corners = torch.stack([lo.double() * s_lo, lo.double() * s_hi, hi.double() * s_lo, hi.double() * s_hi])
            lo, hi = half(corners.amin(0)), half(corners.amax(0))
        if res16 is not None:
            lo, hi = half(add_residual(lo, res16)[0]), half(add_residual(hi, res16)[0])
        g = got16.double()
        ok = torch.where(wide, (g >= lo.double()) & (g <= hi.double()), ok)
    return ok


def epilogue_nominal(ref, gelu=False, res16=None):
    """the epilogue on the correctly rounded v = half(ref) with the correctly rounded sigmoid: fp16"""
    v = half(ref)
    if gelu:
        v = half(quick_gelu(v)[0])
    if res16 is not None:
        v = half(add_residual(v, res16)[0])
    return v


def pool(x, mask, Lw, normalize):
    """MESM.CLIP_encode_text / GloVe_encode_text tail in fp64: the first Lw tokens of x (N, Lx, D), pads zeroed by
    mask (N, Lm) bool cut to Lw the same way, sentence = sum / count of the UN-normalised words, then both L2-normalised
    with the norm clamped at 1e-5.  -> ((words, sent), (e_words, e_sent)), the envelopes of an fp32 evaluation with
    kappa = sqrt(D) + 8 for the D-term norms and Lw + 1 roundings for the sentence's sum and division.  An all-padding
    row gives 0 / 0 = NaN in the sentence and zeros in the words."""
    m = mask[:, :Lw].bool()
    w = x[:, :Lw].double().masked_fill(~m.unsqueeze(-1), 0.0)
    cnt = m.sum(1, keepdim=True).double()
    s = w.sum(1) / cnt
    D = x.shape[-1]
    kappa = math.sqrt(D) + 8.0
    e_s = (Lw + 1) * U32 * (w.abs().sum(1) / cnt)
    e_w = torch.zeros_like(w)
    if normalize:
        wn = w.norm(dim=-1, keepdim=True).clamp_min(1e-5)
        w = w / wn
        e_w = kappa * U32 * w.abs()
        sn = s.norm(dim=-1, keepdim=True).clamp_min(1e-5)
        e_s = (e_s + s.abs() * (e_s.norm(dim=-1, keepdim=True) / sn + kappa * U32)) / sn
        s = s / sn
    return (w, s), (e_w, e_s)


# -------------------------------------------------------------------------------------------------------------- cases
def randn(shape, seed, device="cpu"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32).to(device)


GEMM_SHAPES = [(2464, 1536, 512), (2464, 2048, 512), (2464, 512, 2048), (32, 512, 512), (1, 64, 32), (63, 65, 64),
               (65, 63, 96), (130, 200, 32), (77, 96, 2048)]

# magnitude name -> (std of A, mean of A in stds, std of W times sqrt(K), mean of W in stds, std of the bias).
# The unit-scale operands carry a mean, as the tower's own do (LayerNorm's beta, the residual stream): zero-mean
# operands cancel to sqrt(K) while the envelope follows |A| |W|^T ~ K, and from K = 512 on more than 10 % of the elements
# would have an envelope that spans two fp16 values -- such a case proves nothing.
GEMM_SCALES = {
    "unit": (1.0, 0.35, 1.0, 0.2, 0.5),
    "subnormal": (2.0 ** -8, 0.0, 2.0 ** -7, 0.0, 2.0 ** -16),  # outputs ~3e-5: below the smallest normal fp16 (6.1e-5)
    "overflow": (1.0, 0.0, 30000.0, 0.0, 100.0),  # ~3 % of the outputs beyond 65504
}


def gemm_operands(M, N, K, scale="unit", a_f32=False, seed=0, device="cpu"):
    """-> A (fp16, or fp32 values that fp16 cannot hold), W fp16, bias fp16"""
    sa, ma, sw, mw, sb = GEMM_SCALES[scale]
    A = (randn((M, K), 1000 + seed, device) + ma) * sa
    W = ((randn((N, K), 2000 + seed, device) + mw) * (sw / math.sqrt(K))).half()
    b = (randn((N,), 3000 + seed, device) * sb).half()
    if not a_f32:
        A = A.half()
    return A, W, b


LINEAR_SWEEP = [(M, N, K, "unit") for (M, N, K) in GEMM_SHAPES] + \
               [(63, 65, 64, "subnormal"), (130, 200, 32, "overflow"), (77, 96, 2048, "subnormal"),
                (65, 63, 96, "overflow")]

LN_SHAPES = [(2464, 512), (77, 64), (1, 32), (5, 96), (7, 100), (300, 2048), (13, 2112)]
