"""The five kernels of csrc/clip_text.hip, each on its own against the fp64 reference of tests/f16_ref.py (evaluated on the
CPU on the operands the kernel read), at the shapes, strides and magnitudes where a tile loop or a rounding goes wrong.

GEMM and LayerNorm cases are held to three criteria:
  (a) every output element is an accepted fp16 value of its envelope (f16_ref.inside / epilogue_accepts);
  (b) the share of elements that differ from the correctly rounded fp64 result is at most 4 x the share the reference's
      own fp32 evaluation on the CPU (blocked accumulation in the kernel's order; F.layer_norm) shows on the same case,
      with a floor of 8 elements -- a systematic double rounding moves several percent of the elements while each stays
      "one step away";
  (c) no NaN where the reference has none, +-inf exactly where the reference's fp16 result is +-inf.
Each case prints `CASE <name> c=<measured c of the CPU evaluation> device_neq=<share> cpu_neq=<share> ambiguous=<share>`
and fails when more than 10 % of its envelopes hold two fp16 values (such a case proves nothing).

mesm_amd.kernels.gemm_f16 allocates its output, so writes outside an M x N window are checked through the C entry point
with a poisoned, wider buffer (test_gemm_f16_writes_only_its_window).

Besides f16_ref.py, attn_ref.py and torch, the pooling tests import oracle/clip_text_oracle.py (in this repository, torch
only): the bound of text_pool is set by the error of the oracle's own `_pool` in fp32, and the all-padding row is pinned
to it.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import f16_ref as R

pytestmark = pytest.mark.gpu
AMBIGUOUS_CAP = 0.10
BLOCK_GEMM_AMBIGUOUS_CAP = 0.20  # the GEMM stages of the residual block: see test_residual_block_stage_by_stage


def dev():
    return torch.device("cuda:0")


def report(name, c, dev_neq, cpu_neq, n, amb, cap=AMBIGUOUS_CAP):
    print("CASE %s c=%.3f device_neq=%.5f cpu_neq=%.5f n=%d ambiguous=%.4f" % (name, c, dev_neq / n, cpu_neq / n, n, amb))
    assert dev_neq <= max(4 * cpu_neq, 8), (name, "criterion (b)", dev_neq, cpu_neq)
    assert amb <= cap, (name, "ambiguous share", amb, cap)


def check_nonfinite(name, got, nominal):
    """criterion (c)"""
    assert not bool((torch.isnan(got) & ~torch.isnan(nominal)).any()), (name, "NaN where the reference has none")
    for inf in (float("inf"), -float("inf")):
        assert torch.equal(got == inf, nominal == inf), (name, "inf", inf)


# ---------------------------------------------------------------------------------------------------------------- GEMM
@functools.lru_cache(maxsize=16)
def operands(M, N, K, scale):
    """CPU operands of one case and the blocked fp32 accumulation of A W^T (the fp16 and the fp32 A share it: the fp32
    one is rounded to the fp16 one while staged).  A32's values are not fp16 values."""
    A32, W, b = R.gemm_operands(M, N, K, scale, a_f32=True, seed=M + N + K)
    assert not torch.equal(A32.half().float(), A32)
    return A32, W, b, R.blocked_f32_accumulate(A32, W)


def eager_epilogue(v16, gelu, res):
    """the eager fp16 tensor ops of the tower on the CPU (fp32 inside, one rounding per op)"""
    if gelu:
        v16 = v16 * torch.sigmoid(1.702 * v16)
    if res is not None:
        v16 = res + v16
    return v16


def check_gemm(name, got, A, W, bias, acc=None, gelu=False, res=None, cap=AMBIGUOUS_CAP):
    """got: the kernel's output on the CPU (fp16, or fp32 holding fp16 values); A, W, bias, res: what it read (CPU)."""
    if got.dtype == torch.float32:
        assert torch.equal(got.half().float(), got) or bool(torch.isnan(got).any()), (name, "fp32 output is not fp16 values")
        got = got.half()
    ref, e = R.linear(A, W, bias)
    blk = R.blocked_f32_linear(A, W, bias, acc)
    c = float(((blk.double() - ref).abs() / (e / R.C_LIN).clamp_min(1e-300)).max())
    nominal = R.epilogue_nominal(ref, gelu, res)
    cpu = eager_epilogue(blk.half(), gelu, res)
    ok = R.epilogue_accepts(got, ref, e, gelu, res)
    n_bad = int((~ok).sum())
    if n_bad:
        i = tuple(int(t[0]) for t in torch.nonzero(~ok, as_tuple=True))
        lo, hi = R.interval(ref, e)
        print("REJECTED %s: %d of %d, first at %s: got %r, v in [%r, %r], nominal %r" % (
            name, n_bad, ok.numel(), i, got[i].item(), lo[i].item(), hi[i].item(), nominal[i].item()))
    check_nonfinite(name, got, nominal)
    report(name, c, int((~R.same16(got, nominal)).sum()), int((~R.same16(cpu, nominal)).sum()), ok.numel(),
           float(R.ambiguous(ref, e).double().mean()), cap)
    assert n_bad == 0, (name, "criterion (a)", n_bad)


def run_gemm(A, W, bias, res=None, gelu=False, out_f32=False):
    from mesm_amd import kernels as kn
    d = dev()
    out = kn.gemm_f16(A.to(d), W.to(d), None if bias is None else bias.to(d), residual=None if res is None else res.to(d),
                      out_f32=out_f32, quick_gelu=gelu)
    assert out.dtype == (torch.float32 if out_f32 else torch.float16) and out.shape == (A.shape[0], W.shape[0])
    return out.cpu()


def residual_for(M, N, scale=2.0, seed=77):
    return (R.randn((M, N), seed) * scale).half()


@pytest.mark.parametrize("a_f32", [False, True])
@pytest.mark.parametrize("M,N,K", R.GEMM_SHAPES)
def test_gemm_f16_shapes(M, N, K, a_f32):
    A32, W, b, acc = operands(M, N, K, "unit")
    A = A32 if a_f32 else A32.half()
    bias = None if (M, N, K) == (32, 512, 512) else b  # the pooled projection has none
    got = run_gemm(A, W, bias)
    got32 = run_gemm(A, W, bias, out_f32=True)
    assert torch.equal(got32, got.float())  # the same fp16 values, widened
    check_gemm("gemm %dx%dx%d %s" % (M, N, K, "f32A" if a_f32 else "f16A"), got, A, W, bias, acc)


EPILOGUES = {"gelu": (True, False), "res": (False, True), "gelu+res": (True, True)}
EPI_CASES = [(M, N, K, epi, a_f32) for (M, N, K) in [(63, 65, 64), (65, 63, 96), (130, 200, 32), (1, 64, 32)]
             for epi in EPILOGUES for a_f32 in (False, True)] + \
            [(2464, 2048, 512, "gelu", False), (2464, 512, 2048, "res", False), (2464, 1536, 512, "gelu+res", True),
             (77, 96, 2048, "gelu+res", False), (32, 512, 512, "res", True)]


@pytest.mark.parametrize("M,N,K,epi,a_f32", EPI_CASES)
def test_gemm_f16_epilogues(M, N, K, epi, a_f32):
    """bias + QuickGELU, bias + residual, and both (the kernel allows it; the tower does not use it)"""
    gelu, with_res = EPILOGUES[epi]
    A32, W, b, acc = operands(M, N, K, "unit")
    A = A32 if a_f32 else A32.half()
    res = residual_for(M, N) if with_res else None
    got = run_gemm(A, W, b, res, gelu)
    got32 = run_gemm(A, W, b, res, gelu, out_f32=True)
    assert torch.equal(got32, got.float())
    check_gemm("gemm %dx%dx%d %s %s" % (M, N, K, epi, "f32A" if a_f32 else "f16A"), got, A, W, b, acc, gelu, res)


@pytest.mark.parametrize("a_f32", [False, True])
@pytest.mark.parametrize("M,N,K", [(65, 63, 96), (130, 200, 32), (77, 96, 2048)])
def test_gemm_f16_strided_operands(M, N, K, a_f32):
    """A as a column slice of a wider tensor (lda > K, base 16-byte aligned), W as a row slice of a taller one, the
    residual with ldr > N"""
    from mesm_amd import kernels as kn
    A32, W, b, acc = operands(M, N, K, "unit")
    A = A32 if a_f32 else A32.half()
    res = residual_for(M, N)
    d = dev()
    off = 4 if a_f32 else 8  # 16 bytes
    Awide = torch.full((M, K + 24), 1e4, dtype=A.dtype, device=d)
    Awide[:, off:off + K] = A.to(d)
    Wtall = torch.full((3 * N, K), -1e4, dtype=torch.float16, device=d)
    Wtall[N:2 * N] = W.to(d)
    Rwide = torch.full((M, N + 5), 3e4, dtype=torch.float16, device=d)
    Rwide[:, 2:2 + N] = res.to(d)
    a, w, r = Awide[:, off:off + K], Wtall[N:2 * N], Rwide[:, 2:2 + N]
    assert a.stride(0) == K + 24 and a.data_ptr() % 16 == 0 and r.stride(0) == N + 5
    got = kn.gemm_f16(a, w, b.to(d), residual=r).cpu()
    assert torch.equal(got, run_gemm(A, W, b, res))  # the strides change nothing
    check_gemm("gemm %dx%dx%d strided %s" % (M, N, K, "f32A" if a_f32 else "f16A"), got, A, W, b, acc, False, res)


POISON16, POISON32 = 0x7BCD, 0x7F8BCDEF
EINVAL, EALIGN = -1, -2  # include/mesm_gfx950.h


def raw_gemm(A, W, bias, res, Cview, out_f32, M, N, K, gelu=False, lda=None):
    """the C entry point on an output view the caller owns -> status"""
    from mesm_amd._lib import lib, ptr, stream_ptr
    rc = lib().mesm_gemm_f16(ptr(A), 1 if A.dtype == torch.float32 else 0, A.stride(0) if lda is None else lda, ptr(W),
                             W.stride(0), ptr(bias), ptr(res), res.stride(0) if res is not None else 0, ptr(Cview),
                             1 if out_f32 else 0, Cview.stride(0), M, N, K, 1 if gelu else 0, stream_ptr())
    torch.cuda.synchronize()
    return rc


def poisoned(rows, cols, out_f32):
    if out_f32:
        return torch.full((rows, cols), POISON32, dtype=torch.int32, device=dev()).view(torch.float32)
    return torch.full((rows, cols), POISON16, dtype=torch.int16, device=dev()).view(torch.float16)


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("M,N,K", [(1, 64, 32), (63, 65, 64), (65, 63, 96), (130, 200, 32), (32, 512, 512)])
def test_gemm_f16_writes_only_its_window(M, N, K, out_f32):
    """an M x N window (ldc > N) of a poisoned buffer: the window holds what the wrapper returns, and no bit outside it
    changed -- the rows past M and the columns past N of the last tiles are not stored"""
    A32, W, b, _ = operands(M, N, K, "unit")
    d = dev()
    A, Wd, bd = A32.half().to(d), W.to(d), b.to(d)
    res = residual_for(M, N).to(d)
    buf = poisoned(M + 3, N + 7, out_f32)
    view = buf[2:2 + M, 3:3 + N]
    assert raw_gemm(A, Wd, bd, res, view, out_f32, M, N, K, gelu=True) == 0
    want = run_gemm(A32.half(), W, b, res.cpu(), True, out_f32)
    assert torch.equal(bits(view.cpu().contiguous()), bits(want))
    outside = torch.ones(M + 3, N + 7, dtype=torch.bool)
    outside[2:2 + M, 3:3 + N] = False
    assert bool((bits(buf).cpu()[outside] == (POISON32 if out_f32 else POISON16)).all())


MAGNITUDE_CASES = [(63, 65, 64, "subnormal"), (77, 96, 2048, "subnormal"), (130, 200, 32, "overflow"),
                   (65, 63, 96, "overflow")]


@pytest.mark.parametrize("epi", ["bias", "res", "gelu"])
@pytest.mark.parametrize("M,N,K,scale", MAGNITUDE_CASES)
def test_gemm_f16_magnitudes(M, N, K, scale, epi):
    """outputs in the fp16 subnormal range (below 6.1e-5), and outputs of which some overflow fp16: +-inf there and only
    there; QuickGELU of -inf is -inf * 0 = NaN in the reference too"""
    A32, W, b, acc = operands(M, N, K, scale)
    A = A32.half()
    gelu = epi == "gelu"
    res = residual_for(M, N, 2.0 ** -15 if scale == "subnormal" else 1000.0) if epi == "res" else None
    hr = R.half(R.linear(A, W, b)[0])
    if scale == "subnormal":
        assert float((hr.double().abs() < 2.0 ** -14).double().mean()) > 0.5
    else:
        assert 0 < int(torch.isinf(hr).sum()) < hr.numel() // 4
    got = run_gemm(A, W, b, res, gelu)
    check_gemm("gemm %dx%dx%d %s %s" % (M, N, K, scale, epi), got, A, W, b, acc, gelu, res)


@pytest.mark.parametrize("span,a_scale,w_scale", [(12.0, 0.05, 1.0), (60000.0, 1.0, 30.0)])
def test_gemm_f16_quick_gelu_sweep(span, a_scale, w_scale):
    """v = acc + bias sweeps [-span, span] along the columns: around zero, through the minimum of QuickGELU, and into both
    saturated ends of the sigmoid (s = 0: the output is -0; s = 1: the output is v)"""
    M, N, K = 65, 1000, 32
    A = (R.randn((M, K), 11) * a_scale).half()
    W = (R.randn((N, K), 12) * (w_scale / K ** 0.5)).half()
    b = torch.linspace(-span, span, N).half()
    got = run_gemm(A, W, b, gelu=True)
    v = R.half(R.linear(A, W, b)[0])
    s = R.half(R.quick_gelu_parts(v)[1])
    assert bool((s == 0).any()) and bool((s == 1).any()) and bool(((s > 0) & (s < 1)).any())
    check_gemm("gemm quick_gelu sweep +-%g" % span, got, A, W, b, None, True)


def test_gemm_f16_refuses_what_it_cannot_load():
    """K not a multiple of 32, a base address off 16 bytes, a leading dimension off 8 elements: the wrapper raises, the
    entry point returns a status, and nothing is launched (the poisoned output keeps every bit)"""
    from mesm_amd import kernels as kn
    from mesm_amd._lib import MesmError
    d = dev()
    M, N = 16, 64
    W40, W64 = torch.zeros(N, 40, dtype=torch.float16, device=d), torch.zeros(N, 64, dtype=torch.float16, device=d)
    flat = torch.zeros(M * 64 + 8, dtype=torch.float16, device=d)
    off4 = flat[4:4 + M * 64].view(M, 64)  # base offset by 4 halfs = 8 bytes
    wide = torch.zeros(M, 68, dtype=torch.float16, device=d)[:, :64]  # lda = 68
    cases = [("K = 40", torch.zeros(M, 40, dtype=torch.float16, device=d), W40, EINVAL),
             ("A base + 4 halfs", off4, W64, EALIGN), ("lda = 68", wide, W64, EALIGN)]
    assert off4.data_ptr() % 16 == 8 and wide.stride(0) % 8 == 4
    for name, A, W, status in cases:
        with pytest.raises(MesmError):
            kn.gemm_f16(A, W)
        buf = poisoned(M, N, False)
        assert raw_gemm(A, W, None, None, buf, False, M, N, A.shape[1]) == status, name
        assert bool((bits(buf) == POISON16).all()), name


# ----------------------------------------------------------------------------------------------------------- LayerNorm
def ln_rows(rows, D):
    """fp16 rows N(0.3, 1.5) with the edge rows where there is room: [1] one element at 6e4 among small ones; and, from 64
    rows on (their envelopes are as wide as their conditioning is bad, so they must stay a small share of the case),
    [0] a constant row (variance 0) and [2] a mean of 1000 against a spread of 1 -- a one-pass variance fails there."""
    x = (R.randn((rows, D), 10 * D) * 1.5 + 0.3).half()
    edges = {}
    if rows >= 3:
        x[1] = (R.randn((D,), 10 * D + 5) * 0.5).half()
        x[1, D // 3] = 6e4
        edges["outlier"] = 1
    if rows >= 64:
        x[0] = -2.8125  # 45/16: every partial sum of D of them is exact in fp32
        x[2] = (R.randn((D,), 10 * D + 6) + 1000.0).half()
        edges.update(constant=0, mean=2)
    gamma = 1.0 + 0.1 * R.randn((D,), 10 * D + 1)
    beta = 0.1 * R.randn((D,), 10 * D + 2)
    return x, gamma, beta, edges


def check_ln(name, got, x, gamma, beta, cap=AMBIGUOUS_CAP):
    y, e = R.layernorm(x, gamma, beta, 1e-5)
    y32 = F.layer_norm(x.float(), (x.shape[-1],), gamma, beta, 1e-5)
    nominal = R.half(y)
    ok = R.inside(got, y, e)
    n_bad = int((~ok).sum())
    if n_bad:
        i = tuple(int(t[0]) for t in torch.nonzero(~ok, as_tuple=True))
        print("REJECTED %s: %d of %d, first at %s: got %r, ref %r +- %r" % (name, n_bad, ok.numel(), i, got[i].item(),
                                                                         y[i].item(), e[i].item()))
    check_nonfinite(name, got, nominal)
    report(name, float(((y32.double() - y).abs() / e).max()), int((~R.same16(got, nominal)).sum()),
           int((~R.same16(y32.half(), nominal)).sum()), ok.numel(), float(R.ambiguous(y, e).double().mean()), cap)
    assert n_bad == 0, (name, "criterion (a)", n_bad)


@pytest.mark.parametrize("rows,D", R.LN_SHAPES)
def test_layernorm_f16(rows, D):
    """rows that are and are not a multiple of the 4 per workgroup, D that is and is not a multiple of the 64 lanes
    (`c` in the CASE line is the CPU fp32 LayerNorm's largest error in units of the envelope)"""
    from mesm_amd import kernels as kn
    x, gamma, beta, edges = ln_rows(rows, D)
    d = dev()
    xd = torch.full((rows + 1, D), float("nan"), dtype=torch.float16, device=d)  # a NaN row behind the last one
    xd[:rows] = x.to(d)
    got = kn.layernorm_f16(xd[:rows], gamma.to(d), beta.to(d)).cpu()
    assert got.dtype == torch.float16 and got.shape == x.shape
    check_ln("layernorm %dx%d" % (rows, D), got, x, gamma, beta)
    if "constant" in edges:
        # the mean of D equal, exactly summable values is that value (IEEE division), d = 0, y = beta rounded
        assert torch.equal(bits(got[edges["constant"]]), bits(beta.half()))
    if "mean" in edges:
        y, e = R.layernorm(x, gamma, beta, 1e-5)
        xf = x[edges["mean"]].float()
        m = xf.mean()
        one = ((xf - m) * torch.rsqrt((xf * xf).mean() - m * m + 1e-5) * gamma + beta).half()  # E[x^2] - m^2 in fp32
        r = edges["mean"]
        assert float((~R.inside(one, y[r], e[r])).double().mean()) > 0.5  # the row does tell the two forms apart


@pytest.mark.parametrize("rows,D", [(9, 100), (5, 96), (6, 32), (13, 2112), (4, 512)])
def test_layernorm_f16_of_constant_rows_is_beta(rows, D):
    """variance 0: every row holds one value k/16 whose partial sums are exact in fp32 in any order, the mean is that
    value (IEEE division), d = 0 and y = beta rounded -- exactly, whatever rstd = 1 / sqrt(eps) multiplies.  (The envelope
    of such a row is wide, an inexact mean would be multiplied by 316, so the exact statement is the test; no share is
    reported.)"""
    from mesm_amd import kernels as kn
    consts = torch.tensor([0.0, 1.0, -2.8125, 17.5, -0.0625, 127.9375, -1000.0, 3.0, 0.5, -7.25, 60.0, 2.0, -2.0])[:rows]
    x = consts[:, None].expand(rows, D).contiguous().half()
    assert torch.equal(x.float(), consts[:, None].expand(rows, D))
    gamma = 1.0 + 0.1 * R.randn((D,), 3)
    beta = R.randn((D,), 4)
    d = dev()
    got = kn.layernorm_f16(x.to(d), gamma.to(d), beta.to(d)).cpu()
    y, e = R.layernorm(x, gamma, beta, 1e-5)
    assert torch.equal(y, beta.double().expand(rows, D)) and bool(R.inside(got, y, e).all())
    assert torch.equal(bits(got), bits(beta.half().expand(rows, D).contiguous()))


# ---------------------------------------------------------------------------------------------------------- embeddings
def tables(V, L, D, seed):
    tok = R.randn((V, D), seed) * 0.2
    pos = R.randn((L, D), seed + 1) * 0.1
    tok[V // 2] *= 2.0 ** -13  # fp16-subnormal entries
    assert not torch.equal(tok.half().float(), tok) and not torch.equal(pos.half().float(), pos)
    return tok, pos


@pytest.mark.parametrize("N,L,D", [(3, 5, 300), (4, 7, 64), (2, 77, 512), (5, 3, 1000)])
def test_clip_embed_is_bit_exact(N, L, D):
    """N > 1 and N != L, so `row % L` picks the positional row; D below, above and off a multiple of the 256 threads"""
    from mesm_amd import kernels as kn
    V = 50
    tok, pos = tables(V, L, D, 100 + D)
    g = torch.Generator().manual_seed(D)
    ids = torch.randint(0, V, (N, L), generator=g)
    ids[0, 0], ids[-1, -1], ids[0, 1] = 0, V - 1, V // 2
    d = dev()
    got = kn.clip_embed(ids.to(d), tok.to(d), pos.to(d)).cpu()
    want = R.half(R.embed(ids, tok, pos)[0])
    assert got.dtype == torch.float16 and torch.equal(bits(got), bits(want))


def test_clip_embed_clamps_ids_outside_the_table():
    """This build's behaviour (clip_embed_kernel: id < 0 -> 0, id >= vocab -> vocab - 1); the reference would raise."""
    from mesm_amd import kernels as kn
    V, L, D, N = 20, 4, 96, 3
    tok, pos = tables(V, L, D, 7)
    ids = torch.tensor([[-1, V, 3, -(2 ** 40)], [V + 5, 0, V - 1, 2 ** 40], [1, 2, 3, 4]])
    d = dev()
    got = kn.clip_embed(ids.to(d), tok.to(d), pos.to(d)).cpu()
    want = R.half(R.embed(ids.clamp(0, V - 1), tok, pos)[0])
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("shape,D", [((3, 5), 300), ((7,), 64), ((2, 3, 4), 1000), ((6, 16), 256)])
def test_embed_rows_is_bit_exact(shape, D):
    from mesm_amd import kernels as kn
    V = 40
    tab = R.randn((V, D), 300 + D)
    tab[1] *= 1e-41  # fp32 subnormals
    tab[2, ::2] = -0.0
    tab[2, 1::2] = 0.0
    tab[3, 0], tab[3, 1] = float("inf"), 2.0 ** -149
    assert not torch.equal(tab.half().float(), tab) and bool((tab[1] != 0).any())
    g = torch.Generator().manual_seed(D)
    ids = torch.randint(0, V, shape, generator=g)
    flat = ids.view(-1)
    flat[0], flat[1], flat[2], flat[3], flat[-1] = 0, V - 1, 1, 2, 3
    d = dev()
    got = kn.embed_rows(ids.to(d), tab.to(d)).cpu()
    assert got.shape == shape + (D,) and got.dtype == torch.float32
    assert torch.equal(bits(got), bits(tab[ids]))


def test_embed_rows_clamps_ids_outside_the_table():
    """This build's behaviour (embed_rows_kernel: id < 0 -> 0, id >= vocab -> vocab - 1); nn.Embedding would raise."""
    from mesm_amd import kernels as kn
    V, D = 11, 300
    tab = R.randn((V, D), 9)
    ids = torch.tensor([[-1, V, 5], [V + 100, -7, V - 1]])
    d = dev()
    got = kn.embed_rows(ids.to(d), tab.to(d)).cpu()
    assert torch.equal(bits(got), bits(tab[ids.clamp(0, V - 1)]))


# ------------------------------------------------------------------------------------------------------------- pooling
def pool_inputs(N, Lx, Lm, Lw, D, dtype, seed):
    """x and ONE mask (N, Lm) for the case; the kernel and the reference cut both to Lw as MESM.CLIP_encode_text does.
    Row 0 has one valid word, row 1 is full, row 2 has a valid word of zeros; every padded position of x holds inf or
    NaN, inside the first Lw tokens and beyond."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, Lx, D, generator=g) * 0.7).to(dtype)
    n_valid = torch.randint(2, Lw + 1, (N,), generator=g)
    n_valid[0], n_valid[1] = 1, Lw
    mask = torch.arange(Lm)[None, :] < n_valid[:, None]
    if Lm > Lw:
        mask[:, Lw:] = torch.rand(N, Lm - Lw, generator=g) < 0.5  # beyond the cut: must not matter
    x[2, 1] = 0.0
    pad = ~F.pad(mask[:, :min(Lm, Lx)], (0, max(0, Lx - Lm)), value=False)
    junk = torch.tensor([float("inf"), -float("inf"), float("nan")]).to(dtype)
    x[pad] = junk[torch.randint(0, 3, (int(pad.sum()), D), generator=g)]
    return x, mask


def check_pool(name, got_w, got_s, x, mask, Lw, normalize, rows=None):
    from oracle import clip_text_oracle as C
    (w, s), _ = R.pool(x, mask, Lw, normalize)
    w32, s32 = C._pool(x.float()[:, :Lw], mask[:, :Lw], normalize)  # the oracle's fp32 evaluation on the CPU
    rows = list(range(x.shape[0])) if rows is None else rows
    pads = ~mask[:, :Lw]
    assert float(got_w[pads].abs().max()) == 0.0 if bool(pads.any()) else True, (name, "padded words are not zero")
    for what, got, ref, cpu in (("words", got_w, w, w32), ("sentence", got_s, s, s32)):
        assert bool(torch.isfinite(got[rows]).all()), (name, what)
        err = float((got.double() - ref)[rows].abs().max())
        cpu_err = float((cpu.double() - ref)[rows].abs().max())
        print("POOL %s %s: device error %.3g, CPU fp32 error %.3g" % (name, what, err, cpu_err))
        assert err <= 4.0 * cpu_err, (name, what, err, cpu_err)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("Lx,Lm,Lw,D", [(20, 24, 16, 300), (16, 16, 16, 512), (77, 32, 32, 64), (12, 77, 12, 1000)])
def test_text_pool(Lx, Lm, Lw, D, dtype, normalize):
    """Lx > Lw and == Lw, Lm > Lw and == Lw; D wraps the 256-thread column loop (300, 512, 1000) and the 64-lane row loop"""
    from mesm_amd import kernels as kn
    N = 6
    x, mask = pool_inputs(N, Lx, Lm, Lw, D, dtype, 1000 + D)
    d = dev()
    w, s = kn.text_pool(x.to(d), mask.to(d), Lw, normalize)
    assert w.shape == (N, Lw, D) and s.shape == (N, D) and w.dtype == s.dtype == torch.float32
    check_pool("%s Lx%d Lm%d Lw%d D%d %s" % (str(dtype)[6:], Lx, Lm, Lw, D, "normalized" if normalize else "plain"),
               w.cpu(), s.cpu(), x, mask, Lw, normalize)


@pytest.mark.parametrize("normalize", [True, False])
def test_text_pool_of_an_all_padding_row_is_the_oracles(normalize):
    """pinned to oracle _pool: 0 / 0 = NaN in the sentence feature of that row, zeros in its words; the other rows are
    untouched by it"""
    from mesm_amd import kernels as kn
    from oracle import clip_text_oracle as C
    N, Lx, Lm, Lw, D = 4, 20, 20, 16, 300
    x, mask = pool_inputs(N, Lx, Lm, Lw, D, torch.float16, 5)
    mask[3, :Lw] = False
    d = dev()
    w, s = kn.text_pool(x.to(d), mask.to(d), Lw, normalize)
    w, s = w.cpu(), s.cpu()
    wo, so = C._pool(x.float()[:, :Lw].masked_fill(~mask[:, :Lw, None], 0.0), mask[:, :Lw], normalize)
    assert torch.isnan(so[3]).all() and float(wo[3].abs().max()) == 0.0
    assert torch.isnan(s[3]).all() and float(w[3].abs().max()) == 0.0
    check_pool("all-padding row %s" % normalize, w, s, x, mask, Lw, normalize, rows=[0, 1, 2])


# ------------------------------------------------------------------------------------- one residual block, by stage
def test_residual_block_stage_by_stage():
    """ResidualAttentionBlock(512, 8) on 32 x 77 rows with the weight statistics of
    test_full_size_clip_tower_against_cpu_oracle: each of the seven stages is run through kn.* and held to the f16_ref
    stage evaluated on the DEVICE's own input to it (errors do not compound), the attention core to attn_ref with its
    causal bound; then the module's forward must be the staged chain bit for bit (which tensor is the residual, which
    LayerNorm feeds which GEMM).  The two LayerNorm stages keep the 10 % cap on ambiguous envelopes.  The operands of the four
    GEMM stages are the tower's zero-mean weights, not chosen: with K = 512 and 2048 they cancel to sqrt(K) under an
    envelope of order K, and more than 10 % of the envelopes hold two fp16 values: zero-mean unit-scale operands with
    K = 512 ... 2048 give 10-18 % under this C_LIN on the CPU (profiles/clip_text_kernels/README.md).  Other magnitudes
    cannot be picked here, so the share of these four stages (a property of the operands and the envelope alone, the
    kernel has no part in it) is capped at 20 % (BLOCK_GEMM_AMBIGUOUS_CAP) so that it cannot drift unseen; criteria
    (a)-(c) hold on every element all the same."""
    from attn_ref import attention, causal_mask, row_bounds, row_err
    from mesm_amd import kernels as kn
    from mesm_amd.text_encoder import CLIPTextEncoder
    torch.manual_seed(3)
    enc = CLIPTextEncoder(512, 77, 49408, 512, 8, 1)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if "ln_" in n:
                p.add_(torch.randn_like(p) * 0.1)
            elif n.endswith("bias"):
                p.copy_(torch.randn(p.shape) * 0.05)
            elif "embedding" in n:
                p.mul_(10.0)
    N, L, d, H = 32, 77, 512, 8
    ids = torch.randint(1, 49406, (N, L))
    blk = enc.transformer.resblocks[0]
    cpu = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    x = (enc.token_embedding.weight[ids].half() + enc.positional_embedding.half()).detach()
    blk = blk.to(dev())
    xd = x.to(dev())
    x2 = xd.view(N * L, d)
    a = blk.attn

    h = kn.layernorm_f16(x2, blk.ln_1.weight, blk.ln_1.bias)
    check_ln("block ln_1", h.cpu(), x.view(N * L, d), cpu["ln_1.weight"], cpu["ln_1.bias"])

    qkv = kn.gemm_f16(h, a.in_proj_weight, a.in_proj_bias, out_f32=True)
    check_gemm("block in_proj", qkv.cpu(), h.cpu(), cpu["attn.in_proj_weight"], cpu["attn.in_proj_bias"],
               cap=BLOCK_GEMM_AMBIGUOUS_CAP)

    qkv3 = qkv.view(N, L, 3 * d)
    q, k, v = qkv3[..., :d], qkv3[..., d:2 * d], qkv3[..., 2 * d:]
    o, _ = kn.attn_fwd(q, k, v, H, causal=True, want_lse=False)
    masked = causal_mask(N, H, L, L)
    scale = (d // H) ** -0.5
    ref, _ = attention(q, k, v, H, masked, scale)
    bound = row_bounds(q, k, v, H, masked, scale, p16=True)["o"]
    r = float((row_err(o, ref, H) / bound).max())
    print("MARGIN block attention o %.3g" % r)
    assert r <= 1.0 and bool(torch.isfinite(o).all())

    o2 = o.view(N * L, d)
    assert o2.dtype == torch.float32
    xa = kn.gemm_f16(o2, a.out_proj.weight, a.out_proj.bias, residual=x2)
    check_gemm("block out_proj + x", xa.cpu(), o2.cpu(), cpu["attn.out_proj.weight"], cpu["attn.out_proj.bias"],
               res=x.view(N * L, d), cap=BLOCK_GEMM_AMBIGUOUS_CAP)

    h2 = kn.layernorm_f16(xa, blk.ln_2.weight, blk.ln_2.bias)
    check_ln("block ln_2", h2.cpu(), xa.cpu(), cpu["ln_2.weight"], cpu["ln_2.bias"])

    f = kn.gemm_f16(h2, blk.mlp.c_fc.weight, blk.mlp.c_fc.bias, quick_gelu=True)
    check_gemm("block c_fc QuickGELU", f.cpu(), h2.cpu(), cpu["mlp.c_fc.weight"], cpu["mlp.c_fc.bias"], gelu=True,
               cap=BLOCK_GEMM_AMBIGUOUS_CAP)

    xo = kn.gemm_f16(f, blk.mlp.c_proj.weight, blk.mlp.c_proj.bias, residual=xa)
    check_gemm("block c_proj + x", xo.cpu(), f.cpu(), cpu["mlp.c_proj.weight"], cpu["mlp.c_proj.bias"], res=xa.cpu(),
               cap=BLOCK_GEMM_AMBIGUOUS_CAP)

    with torch.no_grad():
        whole = blk(xd)
    assert whole.shape == (N, L, d) and torch.equal(bits(whole.view(N * L, d)), bits(xo))
