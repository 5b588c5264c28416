"""fp64 reference of the attention core (MesmAttnArgs, include/mesm_gfx950.h) for every mask option, and the per-row
error bounds the kernels are held to.  Shared by tests/test_attention_options_gpu.py (on the device, fp64) and
tests/test_attn_ref_cpu.py (which pins the masks and the core to oracle/mesm_oracle.py).

Nothing here restates the kernels' own index arithmetic (csrc/common.hpp mesm_quirk_row): the T2V mask comes from
`oracle.mesm_oracle.t2v_mask` -- pinned to the real reference by the golden fixtures -- applied to each group of stacked
rows on its own, and a padded batch is the unpadded batch of its first n rows plus dummy rows under their own masks.
Split heads are plain attention on the interleaved [q || q2], [k + k_add || k2] tensors.
"""
import torch

from oracle.mesm_oracle import t2v_mask

U32 = 2.0 ** -24  # unit roundoff of float32


def heads(x, H):
    """(B, L, H*d) -> (B, H, L, d)"""
    B, L, E = x.shape
    return x.reshape(B, L, H, E // H).transpose(1, 2)


def unheads(x):
    """(B, H, L, d) -> (B, L, H*d)"""
    B, H, L, d = x.shape
    return x.transpose(1, 2).reshape(B, L, H * d)


def interleave(a, b, H):
    """per head [a_h || b_h]: the split-head layout of MesmAttnArgs.q2 / k2 as one packed (B, L, 2*E) tensor"""
    B, L, E = a.shape
    return torch.cat([a.reshape(B, L, H, E // H), b.reshape(B, L, H, E // H)], -1).reshape(B, L, 2 * E)


def split(x, H):
    """inverse of interleave"""
    B, L, E = x.shape
    x4 = x.reshape(B, L, H, E // H)
    h = E // H // 2
    return x4[..., :h].reshape(B, L, E // 2), x4[..., h:].reshape(B, L, E // 2)


def kpad_mask(kpad, H, Lq):
    """(B, Lk) key padding -> (B, H, Lq, Lk)"""
    B, Lk = kpad.shape
    return kpad.bool()[:, None, None, :].expand(B, H, Lq, Lk)


def causal_mask(B, H, Lq, Lk, kpad=None):
    """MESM_MASK_CAUSAL: key j of query i is masked iff j > i, or-ed with the key padding"""
    m = torch.ones(Lq, Lk, dtype=torch.bool).triu(1)[None, None].expand(B, H, Lq, Lk)
    if kpad is not None:
        m = m | kpad_mask(kpad.cpu(), H, Lq)
    return m


def quirk_mask(qpad, kpad, H, group=0, mod=None):
    """MESM_MASK_T2V_QUIRK with mask_group = group (0: one group of B rows) and mask_mod = mod (None: off).
    Each group of G stacked rows is an independent batch of the reference; with a modulus n only its first n rows are
    real pairs (the reference sees the unpadded batch of n) and the dummy rows beyond see their own masks, i.e. their
    key padding alone.  -> (B, H, Lq, Lk) bool, True = masked."""
    qpad, kpad = qpad.bool().cpu(), kpad.bool().cpu()
    B, Lq = qpad.shape
    G = group if group > 0 else B
    assert B % G == 0
    n = G if mod is None else mod
    assert 1 <= n <= G
    out = []
    for s in range(0, B, G):
        out.append(t2v_mask(qpad[s:s + n], kpad[s:s + n], H))
        if n < G:
            out.append(kpad_mask(kpad[s + n:s + G], H, Lq))
    return torch.cat(out)


def attention(q, k, v, H, masked=None, scale=None, drop=None):
    """fp64 attention core on packed (B, L, H*d) tensors: softmax(scale q k^T, -inf where masked (B, H, Lq, Lk)),
    times the dropout multiplier drop (B, H, Lq, Lk) (0 or 1/(1-p); None = off), times v.
    -> o (B, Lq, H*dv), lse (B, H, Lq) = logsumexp of the masked scaled scores.
    A row whose keys are all masked gives NaN in o and -inf in lse (torch.softmax / torch.logsumexp)."""
    qh, kh, vh = heads(q.double(), H), heads(k.double(), H), heads(v.double(), H)
    if scale is None:
        scale = qh.shape[-1] ** -0.5
    s = scale * (qh @ kh.transpose(-1, -2))
    if masked is not None:
        s = s.masked_fill(masked.to(s.device), float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.softmax(s, -1)
    if drop is not None:
        p = p * drop.to(p.device).double()
    return unheads(p @ vh), lse


# ------------------------------------------------------------------------------------------------------- error bounds
# First-order worst-case bounds of a float32 evaluation, per row, in units of U32; dk, dv = head widths, S = the largest
# score magnitude scale * sum_d |q_d k_d| over unmasked pairs, W_i = max over the unmasked keys j of row i of
# max|v_j| * (dropout multiplier).  No accumulation order is assumed (atomics and matrix-core blocks are covered).
#
# forward, row i of o:  o_i = sum_j p_j w_j with w_j = m_j v_j, sum_j p_j = 1, so |o_i| <= W_i, and
#   score rounding      |ds_j| <= (dk + 2) U S        (dk-term dot product, the scale, the k_add sum)
#                       -> |do| <= sum_j p_j |ds_j| |w_j - o| <= 2 (dk + 2) U S W
#   __expf(x)           relative (1.5 |x| + 2) U, with sum_j p_j |x_j| <= Lk / e  -> <= 2 (0.56 Lk + 2) U W
#                       (the online rescale exp(m_old - m_new) scales numerator and denominator alike: cancels)
#   acc = sum e_j w_j, l = sum e_j, o = acc / l, dropout product   -> <= (2 Lk + 2) U W
#   KAPPA_O = 2 (dk + 2) S + 4 Lk + 8.
# MESM_MASK_CAUSAL hands the probabilities to P V rounded to fp16 (the frozen CLIP tower's fp16 SDPA, attention.hip):
#   relative 2^-11 = 8192 U per normal p_j, absolute 2^-25 <= U per subnormal one -> + (8192 + Lk) U W (p16=True).
# lse_i = m + log l: shift of the max <= (dk + 2) U S, log of l <= (1.6 Lk + 2) U, the final rounding U |lse|
#   -> |dlse| <= U (KAPPA_O + 2 |lse_i|).
# backward: the probabilities are recomputed as exp(scale s - lse) with relative error
#   eps_P <= U [(dk + 2) S  +  KAPPA_O  +  1.5 (2 S + ln Lk) + 2]          (x = lse - s <= 2 S + ln Lk)
# dv_j = sum_i P_ij m_ij dO_i: eps_P + (Lq + 1) U of the magnitude sum_i P_ij m_ij |dO_i|.
# dS_ij = P_ij (m_ij dO_i.v_j - D_i), D_i = dO_i.o_i with the forward's o (|o_i - o_ref| <= KAPPA_O U W_i): its
#   error is <= (eps_P + (dv + 2) U + KAPPA_O U) A_ij with A_ij = P_ij (m_ij |dO_i|.|v_j| + |dO_i|_1 W_i);
# dk_j = scale sum_i dS_ij q_i, dq_i = scale sum_j dS_ij k_j: a further (Lq + Lk + 2) U of scale A^T |q|, scale A |k|.
#   KAPPA_B = 4 (dk + 3) S + 10 (Lq + Lk) + 2 dv + 32 covers all three.
# Each gradient row (b, h, key or query) is held to KAPPA_B U max(R_row, 2^-12 R_max), R_row = the largest magnitude of
# the row, R_max that of the tensor: the floor only guards rows whose magnitude underflows.


def kappa_o(dk, Lk, S, p16=False):
    return 2.0 * (dk + 2) * S + 4.0 * Lk + 8.0 + ((8192.0 + Lk) if p16 else 0.0)


def kappa_b(dk, dv, Lq, Lk, S):
    return 4.0 * (dk + 3) * S + 10.0 * (Lq + Lk) + 2.0 * dv + 32.0


def row_bounds(q, k, v, H, masked, scale, drop=None, do=None, p16=False):
    """Per-row error bounds (see above) of o, lse and, with do, of dq, dk, dv; every tensor (B, H, L) with L the row's
    extent (Lq for o / lse / dq, Lk for dk / dv).  q / k / v are the packed (interleaved) fp32 inputs; p16: the
    probabilities are rounded to fp16 before P V (causal forward)."""
    qh, kh, vh = heads(q.double(), H).abs(), heads(k.double(), H).abs(), heads(v.double(), H).abs()
    B, _, Lq, dk = qh.shape
    Lk, dv = kh.shape[2], vh.shape[3]
    masked = masked.to(qh.device)
    mult = torch.ones(B, H, Lq, Lk, dtype=torch.float64, device=qh.device) if drop is None else drop.to(qh.device).double()
    mult = mult.masked_fill(masked, 0.0)
    S = (scale * (qh @ kh.transpose(-1, -2))).masked_fill(masked, 0.0).max().item()
    W = (vh.amax(-1)[:, :, None, :] * mult).amax(-1)  # (B, H, Lq)
    ko = kappa_o(dk, Lk, S)
    _, lse = attention(q, k, v, H, masked, scale)
    out = {"o": kappa_o(dk, Lk, S, p16) * U32 * W, "lse": U32 * (ko + 2.0 * lse.abs())}
    if do is None:
        return out
    s = (scale * (heads(q.double(), H) @ heads(k.double(), H).transpose(-1, -2))).masked_fill(masked, float("-inf"))
    P = torch.softmax(s, -1)
    G = heads(do.double(), H).abs()
    A = P * (mult * (G @ vh.transpose(-1, -2)) + (G.sum(-1) * W)[..., None])
    kb = kappa_b(dk, dv, Lq, Lk, S)
    for name, M in (("dv", (P * mult).transpose(-1, -2) @ G), ("dk", scale * (A.transpose(-1, -2) @ qh)),
                    ("dq", scale * (A @ kh))):
        R = M.amax(-1)
        out[name] = kb * U32 * torch.clamp(R, min=R.max().item() * 2.0 ** -12)
    return out


def row_err(x, ref, H):
    """max |x - ref| over each head row: (B, L, H*d) -> (B, H, L)"""
    return heads((x.double() - ref.double()).abs(), H).amax(-1)
