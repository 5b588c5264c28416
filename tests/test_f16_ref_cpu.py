"""The fp64 reference of the fp16 text-tower kernels (tests/f16_ref.py), on the CPU: its roundings sit where the
expressions of oracle/clip_text_oracle.py put them, its envelopes hold the oracle's own fp32 evaluations, and the
constant of the Linear envelope is the one a blocked fp32 accumulation measures."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f16_ref as R
from oracle import clip_text_oracle as C


def all_fp16():
    return torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.float16)


def test_half_rounds_once_where_torch_rounds_twice():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1 << 20, dtype=torch.float64, generator=g) * \
        torch.logspace(-9, 4.7, 1 << 20, dtype=torch.float64)
    x[:6] = torch.tensor([1 + 2.0 ** -11 + 2.0 ** -30, 1 + 2.0 ** -11, 65519.999, 65520.0, 2.0 ** -25, -2.0 ** -25 * 1.0001],
                         dtype=torch.float64)
    with np.errstate(over="ignore"):
        want = torch.from_numpy(x.numpy().astype(np.float16))  # numpy rounds fp64 -> fp16 directly
    assert torch.equal(R.half(x).view(torch.int16), want.view(torch.int16))
    assert R.half(x[:1]).item() == 1 + 2.0 ** -10 and x[:1].half().item() == 1.0  # the double rounding half() repairs
    assert R.half(torch.tensor([float("inf"), -float("inf")], dtype=torch.float64)).tolist() == [float("inf"), -float("inf")]
    assert torch.isnan(R.half(torch.tensor([float("nan")], dtype=torch.float64))).all()
    f = torch.randn(1000, generator=g)
    assert torch.equal(R.half(f), f.half()) and R.half(f.half()).dtype == torch.float16


def test_next_up_and_candidates_walk_the_fp16_values():
    h = all_fp16()
    fin = torch.isfinite(h)
    up = R.next_up(h)
    srt = torch.sort(h[fin].double()).values.unique()  # (+0 and -0 are one value)
    nxt = dict(zip(srt[:-1].tolist(), srt[1:].tolist()))
    nxt[65504.0] = float("inf")
    assert [nxt[v] for v in h[fin].double().tolist()] == up[fin].double().tolist()
    assert up[h == float("inf")].item() == float("inf") and torch.isnan(up[torch.isnan(h)]).all()
    ref = torch.tensor([1.0, 1.0 + 2.0 ** -11, -3.0, 65519.0, 0.0], dtype=torch.float64)
    e = torch.tensor([0.0, 2.0 ** -20, 2.0 ** -9, 2.0, 2.0 ** -24], dtype=torch.float64)
    c = torch.stack(R.candidates(ref, e, 4)).double()
    assert c[:, 0].tolist() == [1.0] * 4
    assert c[:, 1].tolist() == [1.0, 1 + 2.0 ** -10, 1 + 2.0 ** -10, 1 + 2.0 ** -10]
    assert c[:, 2].tolist() == [-3.001953125, -3.0, -2.998046875, -2.998046875]
    assert c[:, 3].tolist() == [65504.0, float("inf"), float("inf"), float("inf")]
    assert c[:, 4].tolist() == [-2.0 ** -24, 0.0, 2.0 ** -24, 2.0 ** -24]
    assert R.ambiguous(ref, e).tolist() == [False, True, True, True, True]
    with pytest.raises(AssertionError):
        R.candidates(ref, e * 4, 4)


def test_embed_is_the_oracle_expression_bit_for_bit():
    g = torch.Generator().manual_seed(1)
    V, L, D, N = 50, 7, 300, 5
    tok = torch.randn(V, D, generator=g) * 0.2
    pos = torch.randn(L, D, generator=g) * 0.1
    tok[3] *= 2.0 ** -14  # rows whose fp16 values are subnormal
    assert not torch.equal(tok.half().float(), tok) and not torch.equal(pos.half().float(), pos)
    ids = torch.randint(0, V, (N, L), generator=g)
    ids[0, 0], ids[0, 1], ids[1, 2] = 0, V - 1, 3
    want = tok[ids].half() + pos.half()  # clip_text_forward's first line
    v, e = R.embed(ids, tok, pos)
    assert float(e.abs().max()) == 0.0
    assert torch.equal(R.half(v).view(torch.int16), want.view(torch.int16))


def test_quick_gelu_is_the_oracle_expression():
    """f * sigmoid(1.702 * f) on every finite fp16 value.  The oracle's sigmoid is an fp32 one: where its envelope holds
    one fp16 value the helper's nominal result is bit-identical; on the few inputs where the fp32 sigmoid may round to
    either neighbour (5 of 63488 do differ from the correctly rounded one) the oracle's value is an accepted one."""
    f = all_fp16()
    f = f[torch.isfinite(f)]
    want = f * torch.sigmoid(1.702 * f)
    nominal = R.half(R.quick_gelu(f)[0])
    _, sig, es = R.quick_gelu_parts(f)
    one = ~R.ambiguous(sig, es)
    print("sigmoid envelopes holding two fp16 values: %d of %d; oracle != nominal on %d"
          % (int((~one).sum()), f.numel(), int((~R.same16(want, nominal)).sum())))
    assert bool(R.same16(want, nominal)[one].all())
    assert int(one.sum()) > 0.9 * f.numel()
    ok = torch.zeros_like(one)
    for c in R.quick_gelu_candidates(f):
        ok |= R.same16(want, c)
    assert bool(ok.all())
    # t is the fp32 product rounded to fp16, as the eager op forms it
    assert torch.equal(R.quick_gelu_parts(f)[0].view(torch.int16), (1.702 * f).view(torch.int16))
    # the infinities: sigmoid saturates; -inf * 0 is NaN in the oracle and in the helper
    inf = torch.tensor([float("inf"), -float("inf")], dtype=torch.float16)
    assert bool(R.same16(R.half(R.quick_gelu(inf)[0]), inf * torch.sigmoid(1.702 * inf)).all())


def test_add_residual_is_the_oracle_expression_bit_for_bit():
    g = torch.Generator().manual_seed(2)
    h = all_fp16()
    h = h[torch.isfinite(h)]
    x = h[torch.randint(0, h.numel(), (1 << 20,), generator=g)]
    a = h[torch.randint(0, h.numel(), (1 << 20,), generator=g)]
    x = torch.cat([x, h, h])
    a = torch.cat([a, h.flip(0), h.roll(1)])  # x + (-x) and neighbours as well
    v, e = R.add_residual(x, a)
    assert float(e.abs().max()) == 0.0
    assert bool(R.same16(R.half(v), x + a).all())


def ln_case(rows, D, seed=0):
    x = (R.randn((rows, D), 10 * D + seed) * 1.5 + 0.3).half()
    gamma = 1.0 + 0.1 * R.randn((D,), 10 * D + 1)
    beta = 0.1 * R.randn((D,), 10 * D + 2)
    return x, gamma, beta


@pytest.mark.parametrize("rows,D", R.LN_SHAPES)
def test_layernorm_holds_the_oracle_ln_inside_its_envelope(rows, D):
    x, gamma, beta = ln_case(rows, D)
    y, e = R.layernorm(x, gamma, beta, 1e-5)
    want = C._ln(x, gamma, beta)
    assert want.dtype == torch.float16
    assert bool(R.inside(want, y, e).all())
    y32 = F.layer_norm(x.float(), (D,), gamma, beta, 1e-5)
    ratio = float(((y32.double() - y).abs() / e).max())
    amb = float(R.ambiguous(y, e).double().mean())
    neq = float((~R.same16(want, R.half(y))).double().mean())
    print("LN (%d, %d): fp32 error / envelope %.3f, ambiguous %.4f, fp32 != half(ref64) %.5f" % (rows, D, ratio, amb, neq))
    assert ratio <= 1.0 and amb <= 0.10


def test_layernorm_envelope_rejects_a_one_pass_variance_on_a_large_mean():
    x = (R.randn((4, 512), 5) + 1000.0).half()  # spacing 0.5 at 1000: sums are exact in fp32, the kernel's form is too
    gamma, beta = torch.ones(512), torch.zeros(512)
    y, e = R.layernorm(x, gamma, beta, 1e-5)
    xf = x.float()
    two = (xf - xf.mean(-1, keepdim=True)) * torch.rsqrt(xf.var(-1, unbiased=False, keepdim=True) + 1e-5)
    assert bool(R.inside(two.half(), y, e).all())
    m = xf.mean(-1, keepdim=True)
    one = (xf - m) * torch.rsqrt((xf * xf).mean(-1, keepdim=True) - m * m + 1e-5)  # E[x^2] - m^2 in fp32
    assert float((~R.inside(one.half(), y, e)).double().mean()) > 0.5


@pytest.mark.parametrize("a_f32", [False, True])
@pytest.mark.parametrize("M,N,K,scale", [(65, 63, 96, "unit"), (32, 512, 512, "unit"), (63, 65, 64, "subnormal"),
                                         (130, 200, 32, "overflow"), (77, 96, 2048, "unit")])
def test_linear_holds_the_oracle_f_linear_inside_its_envelope(M, N, K, scale, a_f32):
    A, W, b = R.gemm_operands(M, N, K, scale, a_f32, seed=M + N + K)
    if a_f32:
        assert not torch.equal(A.half().float(), A)
    for bias in (b, None):
        ref, e = R.linear(A, W, bias)
        want = F.linear(A.half(), W, bias)  # the oracle's Linear on fp16 tensors
        assert bool(R.inside(want, ref, e).all()), (bias is not None)
        hr = R.half(ref)
        assert torch.equal(torch.isinf(want), torch.isinf(hr)) and not bool(torch.isnan(want).any())
    if scale == "overflow":
        assert 0 < int(torch.isinf(hr).sum()) < hr.numel() // 4
    if scale == "subnormal":
        assert float((hr.abs().double() < 2.0 ** -14).double().mean()) > 0.5


def test_measured_c_of_the_blocked_fp32_linear():
    """The constant of the Linear envelope: the largest |blocked fp32 - fp64| / (2^-24 (|A| |W|^T + |bias|)) over the
    sweep is C_LIN_MEASURED (rounded up to two decimals), and C_LIN is 4 x that."""
    worst = 0.0
    for (M, N, K, scale) in R.LINEAR_SWEEP:
        A, W, b = R.gemm_operands(M, N, K, scale, seed=M + N + K)
        acc = R.blocked_f32_accumulate(A, W)
        for bias in (b, None):
            ref, e = R.linear(A, W, bias)
            blk = R.blocked_f32_linear(A, W, bias, acc)
            unit = e / R.C_LIN  # 2^-24 (|A| |W|^T + |bias|)
            c = float(((blk.double() - ref).abs() / unit.clamp_min(1e-300)).max())
            amb = float(R.ambiguous(ref, e).double().mean())
            neq = float((~R.same16(blk.half(), R.half(ref))).double().mean())
            print("(%d, %d, %d) %s %s: c %.4f, ambiguous at C_LIN %.4f, blocked fp32 != half(ref64) %.5f"
                  % (M, N, K, scale, "bias" if bias is not None else "no bias", c, amb, neq))
            assert bool(R.inside(blk.half(), ref, e / 4.0).all())  # inside the envelope of c = C_LIN_MEASURED itself
            assert amb <= 0.10
            worst = max(worst, c)
    assert R.C_LIN_MEASURED - 0.01 < worst <= R.C_LIN_MEASURED, worst
    assert R.C_LIN == 4.0 * R.C_LIN_MEASURED


def test_blocked_accumulation_is_the_plain_product_in_another_order():
    A, W, b = R.gemm_operands(65, 63, 96, "unit", seed=1)
    blk = R.blocked_f32_linear(A, W, b)
    assert blk.dtype == torch.float32
    want = A.double() @ W.double().t() + b.double()
    assert torch.allclose(blk.double(), want, rtol=0, atol=1e-5)
    # K = 8: one matrix-core product, summed in k order
    a8, w8 = A[:3, :8].float(), W[:2, :8].float()
    seq = torch.zeros(3, 2)
    for k in range(8):
        seq = seq + a8[:, k:k + 1] * w8[:, k][None, :]
    assert torch.equal(R.blocked_f32_accumulate(A[:3, :8], W[:2, :8]), seq)


def test_epilogue_accepts_the_oracle_chain_and_rejects_misplaced_roundings():
    """c_fc -> QuickGELU and c_proj -> + residual as the oracle writes them, on fp16 CPU tensors: accepted.  The same
    chains with a rounding moved (before the bias; none after the residual's first operand; 1.7 for 1.702) are not."""
    M, N, K = 130, 200, 32
    A, W, b = R.gemm_operands(M, N, K, "unit", seed=M + N + K)
    res = (R.randn((M, N), 77) * 2.0).half()
    ref, e = R.linear(A, W, b)
    f = F.linear(A, W, b)
    assert bool(R.epilogue_accepts(f * torch.sigmoid(1.702 * f), ref, e, gelu=True).all())
    assert bool(R.epilogue_accepts(res + f, ref, e, res16=res).all())
    g = f * torch.sigmoid(1.702 * f)
    assert bool(R.epilogue_accepts(res + g, ref, e, gelu=True, res16=res).all())
    nom = R.epilogue_nominal(ref, gelu=True, res16=res)
    assert float((~R.same16(nom, res + g)).double().mean()) < 0.01
    # misplaced roundings: each moves a quarter to a half of the elements out of their accepted sets (0.29, 0.25, 0.47
    # here), far from a lone counterexample; the cap of criterion (b) is broken as well
    acc = R.blocked_f32_linear(A, W, None)
    early = (acc.half().float() + b.float()).half()  # rounded before the bias
    once = (acc + b.float() + res.float()).half()  # the residual added before the only rounding
    g17 = f * torch.sigmoid(1.7 * f)
    cpu_neq = int((~R.same16((acc + b.float()).half(), R.half(ref))).sum())
    for wrong, kw in ((early, {}), (once, dict(res16=res)), (g17, dict(gelu=True))):
        assert float((~R.epilogue_accepts(wrong, ref, e, **kw)).double().mean()) > 0.10
        assert int((~R.same16(wrong, R.epilogue_nominal(ref, **kw))).sum()) > max(4 * cpu_neq, 8)


def test_epilogue_accepts_by_interval_where_the_envelope_is_wide():
    """v next to zero under an envelope of the operands' size: more than 4 fp16 values of v are accepted (2^-24 apart), so
    epilogue_accepts bounds the chain by interval arithmetic there.  Known-good values pass, known-bad ones do not."""
    ref = torch.full((4,), 1e-6, dtype=torch.float64)
    e = torch.full((4,), 3e-6, dtype=torch.float64)
    lo, hi = R.interval(ref, e)
    assert R.candidates(ref, e, 4, strict=False)[1].all() and lo[0].item() < -2e-6 and hi[0].item() > 3.9e-6

    def h(*v):
        return torch.tensor(v, dtype=torch.float16)
    # plain: the interval itself
    got = torch.stack([lo[0], h(0.0)[0], hi[0], R.next_up(hi)[0]])
    assert R.epilogue_accepts(got, ref, e).tolist() == [True, True, True, False]
    assert R.epilogue_accepts(h(-2.2e-6, 1e-6, 4.2e-6, 1.0), ref, e).tolist() == [False, True, False, False]
    # QuickGELU: s = 0.5 next to zero, so the output is v / 2: hi / 2 is accepted, hi itself (a fine v) is not
    got = h(hi[0].item() / 2, 1e-6, hi[0].item(), lo[0].item())
    assert R.epilogue_accepts(got, ref, e, gelu=True).tolist() == [True, True, False, False]
    # residual 1: every accepted v rounds to 1 exactly; the next fp16 value does not pass
    one = torch.ones(4, dtype=torch.float16)
    got = h(1.0, 1.0 + 2.0 ** -10, 1.0 - 2.0 ** -11, 1e-6)
    assert R.epilogue_accepts(got, ref, e, res16=one).tolist() == [True, False, False, False]
    # both: v / 2 + 1
    assert R.epilogue_accepts(got, ref, e, gelu=True, res16=one).tolist() == [True, False, False, False]


def pool_case(N, Lx, Lm, Lw, D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, Lx, D, generator=g) * 0.7).to(dtype)
    n_valid = torch.randint(1, Lw + 1, (N,), generator=g)
    n_valid[0], n_valid[1] = 1, Lw  # one valid word; a full row
    mask = torch.arange(Lm)[None, :] < n_valid[:, None]
    mask[:, Lw:] = torch.rand(N, Lm - Lw, generator=g) < 0.5  # beyond the cut: must not matter
    return x, mask


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_pool_is_the_oracle_pool_to_fp32_rounding(normalize, dtype):
    N, Lx, Lm, Lw, D = 6, 20, 24, 16, 300
    x, mask = pool_case(N, Lx, Lm, Lw, D, dtype, 4)
    x[2, 3] = 0.0  # a valid row of zeros: the norm clamp
    mask[2, 3] = True
    mask[5, :Lw] = False  # an all-padding row
    (w, s), (ew, es) = R.pool(x, mask, Lw, normalize)
    wo, so = C._pool(x.float()[:, :Lw], mask[:, :Lw], normalize)  # as clip_encode_text cuts both
    assert wo.dtype == torch.float32
    assert torch.isnan(so[5]).all() and torch.isnan(s[5]).all() and float(w[5].abs().max()) == 0.0
    assert float(wo[5].abs().max()) == 0.0 and float(w[2, 3].abs().max()) == 0.0
    ok = [0, 1, 2, 3, 4]
    assert bool(((wo.double() - w).abs() <= ew).all())
    assert bool(((so.double() - s).abs()[ok] <= es[ok]).all())
    assert float((wo.double() - w).abs().max()) < 1e-6 and float((so.double() - s)[ok].abs().max()) < 1e-6
    if not normalize:
        assert torch.equal(wo.double(), w)
