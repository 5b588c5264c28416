"""fp64 statement of every loss block of csrc/criterion.hip, csrc/losses.hip and csrc/loss_bodies.hpp, and the error bounds
the kernels are held to.  Shared by tests/test_loss_kernels_gpu.py (on the device, fp64) and tests/test_loss_ref_cpu.py
(which pins every function to oracle/mesm_oracle.py and to tests/ref_losses.py, and shows that the bounds bite).

Plain torch on whatever device the inputs live on, no custom kernel; gradients come from autograd.  Nothing here restates
a kernel's index arithmetic.  Every batch-level function takes n_valid=None: with a count the result is the plain function
on the first n_valid pairs (targets tgt_off[:n_valid + 1], positives pos[:n_valid, :n_valid], every mean over n_valid), so
autograd leaves the gradient rows of the pairs beyond exactly zero.  The padding pairs of a captured capacity are copies of
a real pair (batching.pad_pairs): finite, with valid masks.

Where the reference's max() meets a tie (the argmax correction of `+ 1e-6` inside a log), the first index takes the
gradient, as a serial scan finds it; `first_max` states that without relying on how a torch build breaks ties.

`dt` is float64 everywhere but in tests/test_loss_ref_cpu.py, which evaluates the same statements in float32 to check the
bounds against a second float32 evaluation, and seeds one defect at a time through DEFECTS (empty in every other use).
"""
import torch

U32 = 2.0 ** -24  # unit roundoff of float32
F64 = torch.float64
DEFECTS = set()   # names of seeded defects (tests/test_loss_ref_cpu.py only)
FLOOR = 2.0 ** -12


def _d(name):
    return name in DEFECTS


def first_max(x):
    """row maximum of x (R, n) -> (R, 1), the gradient going to the FIRST index that attains it"""
    n = x.shape[1]
    ar = torch.arange(n, device=x.device).expand_as(x)
    idx = torch.where(x.detach() == x.detach().amax(1, keepdim=True), ar, n).amin(1, keepdim=True)
    return x.gather(1, idx), idx


def lead(k, *ts):
    """every tensor cut to its first k pairs (None stays None)"""
    return [t if t is None else t[:k] for t in ts]


# ----------------------------------------------------------------------------------------------------------- statements
def nll_smooth(logit, label, mask=None, eps=0.1, dt=F64):
    """criterion.py:291-306 per row: logit (R, C), label (R,), mask (R,) bool or None
    -> row_loss (R) (0 where masked), lse (R), correct (R) bool (the FIRST argmax equals the label)."""
    x = logit.to(dt)
    C = x.shape[1]
    lse = torch.logsumexp(x, 1)
    nll = lse - x.gather(1, label[:, None]).squeeze(1)
    smooth = C * lse - x.sum(1)
    loss = (1 - eps) * nll + eps / C * smooth
    if mask is not None:
        loss = loss.masked_fill(~mask.bool(), 0)
    return loss, lse, first_max(x)[1].squeeze(1) == label


def nll_grad(logit, label, lse, row_grad, eps=0.1, dt=F64):
    """d sum_r row_grad_r row_loss_r / d logit in closed form (the row weights already hold the mask)"""
    x, g = logit.to(dt), row_grad.to(dt)[:, None]
    C = x.shape[1]
    p = torch.exp(x - lse.to(dt)[:, None])
    oh = torch.zeros_like(x).scatter_(1, label[:, None], 1.0)
    u = 0.0 if _d("nll_no_eps_over_C") else eps / C
    return g * (p - (1 - eps) * oh - u)


def rec_fw_reduce(row_loss, correct, mask, n_valid=None, dt=F64, _cap=None):
    """criterion.py:293-304: row_loss (N, Lw) with zeros where masked -> (mean over pairs of the masked row mean, accuracy)"""
    if n_valid is not None:
        return rec_fw_reduce(*lead(n_valid, row_loss, correct, mask), dt=dt, _cap=mask.shape[0])
    m = mask.to(dt)
    N = _cap if _cap and _d("recfw_capacity_N") else m.shape[0]  # (_cap: the capacity, for the seeded defect alone)
    loss = ((row_loss.to(dt) * m).sum(1) / m.sum(1)).sum() / N
    return loss, (correct.to(dt) * m).sum() / m.sum()


def rec_fw_rowgrad(mask, g, n_valid=None, dt=F64):
    """d (g x loss of rec_fw_reduce) / d row_loss: g mask / (N x valid words of the pair), (N, Lw)"""
    m = mask.to(dt)
    out = torch.zeros_like(m)
    k = m.shape[0] if n_valid is None else n_valid
    out[:k] = g * m[:k] / (k * m[:k].sum(1, keepdim=True))
    return out


def saliency(s_pos, s_neg, label, vmask, pos_idx, neg_idx, rank_coef, margin, n_valid=None, dt=F64, _cap=None):
    """criterion.py:139-221: s_pos / s_neg (N, L), label (N, L), vmask (N, L) bool, pos_idx / neg_idx (N, P) or None."""
    if n_valid is not None:
        return saliency(*lead(n_valid, s_pos, s_neg, label, vmask, pos_idx, neg_idx), rank_coef, margin, dt=dt,
                        _cap=s_pos.shape[0])
    vm = vmask.to(dt)
    N = s_pos.shape[0]
    den = _cap if _cap and _d("sal_capacity_N") else N
    loss_neg = (-torch.log(1.0 - torch.sigmoid(s_neg.to(dt))) * vm).sum(1).sum() / den
    sc = torch.cat([s_pos.to(dt), s_neg.to(dt)], 1)
    lab = torch.cat([label, torch.zeros_like(label)], 1)
    vm2 = vm.repeat(1, 2)
    cur = (vm2 * sc + (1.0 - vm2) * -1e3) / 0.5
    mx = first_max(cur)[0]
    if _d("sal_no_argmax"):
        mx = mx.detach()
    lg = cur - mx
    lp = lg - torch.log(torch.exp(lg).sum(1, keepdim=True) + 1e-6)
    total = 0.0
    for r in range(1, 12):
        pos = (lab >= r).to(dt)  # (a sum of bools plus 1e-6 would be a float32 tensor)
        if pos.sum() == 0:
            continue
        mlp = (pos * lp * vm2).sum(1) / (pos.sum(1) + 1e-6)
        total = total + (-mlp * (pos.sum(1) > 0)).sum() / N
    total = total / rank_coef + loss_neg
    if pos_idx is not None:
        P = pos_idx.shape[1]
        sp = s_pos.to(dt)
        total = total + torch.clamp(margin + sp.gather(1, neg_idx) - sp.gather(1, pos_idx), min=0).sum() / (N * P) * 2
    return total


def span_cxw_to_xx(s):
    return torch.stack([s[..., 0] - 0.5 * s[..., 1], s[..., 0] + 0.5 * s[..., 1]], -1)


def _clamp0(x, strict):
    """clamp(min=0); strict: the gradient passes for x > 0 only (the seeded defect)"""
    return torch.where(x > 0, x, torch.zeros_like(x)) if strict else x.clamp(min=0)


def _pick(a, b, big, onesided):
    """max(a, b) (big) or min(a, b); onesided: an even tie gives its whole gradient to a (the seeded defect)"""
    if not onesided:
        return torch.max(a, b) if big else torch.min(a, b)
    return torch.where((a >= b) if big else (a <= b), a, b)


def paired_giou(a, b):
    """span_utils.py:92-121 for matched rows: a, b (M, 2) as (start, end)"""
    raw_i = _pick(a[:, 1], b[:, 1], False, _d("giou_onesided_tie")) - _pick(a[:, 0], b[:, 0], True, _d("giou_onesided_tie"))
    inter = _clamp0(raw_i, _d("giou_inter_strict"))
    union = (a[:, 1] - a[:, 0]) + (b[:, 1] - b[:, 0]) - inter
    enc = _clamp0(torch.max(a[:, 1], b[:, 1]) - torch.min(a[:, 0], b[:, 0]), _d("giou_enc_strict"))
    return inter / union - (enc - union) / enc


def matched(tgt_off, match_q, Q):
    """-> (flat (pair x Q + query) index of every matched target, keep (sumT,) bool): matcher.py:108-117 leaves targets
    unmatched (-1) where a pair has more targets than queries"""
    off = tgt_off.long()
    sizes = off[1:] - off[:-1]
    pair_of_t = torch.repeat_interleave(torch.arange(len(sizes), device=off.device), sizes)
    mq = match_q[:int(off[-1])].long()
    keep = mq >= 0
    return (pair_of_t * Q + mq)[keep], keep


def set_losses(logits, spans, tgt_cxw, tgt_xx, tgt_off, match_q, eos_coef, n_valid=None, dt=F64, _cap=None):
    """criterion.py:71-137 given the matching (match_q[t] = query of target t, -1 = unmatched)
    -> (loss_span, loss_giou, loss_label, class_error)."""
    if n_valid is not None:
        return set_losses(logits[:n_valid], spans[:n_valid], tgt_cxw, tgt_xx, tgt_off[:n_valid + 1], match_q, eos_coef, dt=dt,
                          _cap=logits.shape[0])
    N, Q = logits.shape[:2]
    T = int(tgt_off[-1])
    flat, keep = matched(tgt_off, match_q, Q)
    tc, tx = tgt_cxw[:T].to(dt)[keep], tgt_xx[:T].to(dt)[keep]
    src = spans.to(dt).reshape(-1, 2)[flat]
    nm = flat.numel()
    if _d("set_sum_T"):
        nm = T
    loss_span = (src - tc).abs().sum() / (2 * nm)
    loss_giou = (1 - paired_giou(span_cxw_to_xx(src), tx)).sum() / nm
    cls = torch.ones(N * Q, dtype=torch.int64, device=logits.device)
    cls[flat] = 0
    w = torch.tensor([1.0, eos_coef], dtype=dt, device=logits.device)
    if _d("set_eos_on_matched"):
        w = torch.tensor([eos_coef, eos_coef], dtype=dt, device=logits.device)
    lg = logits.to(dt).reshape(N * Q, 2)
    ce = -torch.log_softmax(lg, -1).gather(1, cls[:, None]).squeeze(1) * w[cls]
    picked = lg.detach()[flat]
    ok = (picked[:, 0] >= picked[:, 1]).to(dt).sum()  # argmax == 0, the first index winning a tie
    Nd = _cap if _cap and _d("set_capacity_N") else N
    return loss_span, loss_giou, ce.sum() / (Nd * Q), 100 - ok * (100.0 / flat.numel())


def rec_ss(pv, cmask, ew, wmask, pos, tau, n_valid=None, dt=F64, _cap=None):
    """criterion.py:240-273 -> dict(loss, cn (N, D), wn (N, D), sim (N, N) = cn wn^T / tau, rows (N) per-row terms)."""
    if n_valid is not None:
        k = n_valid
        return rec_ss(pv[:k], cmask[:k], ew[:k], wmask[:k], pos[:k, :k], tau, dt=dt, _cap=pv.shape[0])
    cm, wm = cmask.to(dt).unsqueeze(-1), wmask.to(dt).unsqueeze(-1)
    clip = (pv.to(dt) * cm).sum(1) / cm.sum(1)
    wf = (ew.to(dt) * wm).sum(1) / wm.sum(1)
    cn = torch.nn.functional.normalize(clip, dim=-1)
    wn = torch.nn.functional.normalize(wf, dim=-1)
    sim = cn @ wn.t() / tau
    if _cap and _cap > pos.shape[0] and _d("ss_padding_column"):  # (the first padding pair, a copy of pair 0, stays a column)
        sim = torch.cat([sim, sim[:, :1]], 1)
    mx = first_max(sim)[0]
    if _d("ss_no_argmax"):
        mx = mx.detach()
    lg = sim - mx
    logp = lg - torch.log(torch.exp(lg).sum(1, keepdim=True) + (0.0 if _d("ss_no_1e-6") else 1e-6))
    N = pos.shape[0]
    p = pos.to(dt)
    rows = -(p * logp[:, :N]).sum(1) / (p.sum(1) + 1e-6)
    return dict(loss=rows.sum() / (_cap if _cap and _d("ss_capacity_N") else N), cn=cn, wn=wn, sim=sim[:, :N], rows=rows)


def rowdot(a, b, scale, dt=F64):
    """model.py:301-302: a (N, L, D), b (N, D) -> (N, L)"""
    return (a.to(dt) * b.to(dt).unsqueeze(1)).sum(-1) * scale


def text_prep(x, normalize=True, dt=F64):
    """model.py:145-152 -> words, mask (sum of the normalised features != 0), sentence feature"""
    F = torch.nn.functional
    x = x.to(dt)
    w = F.normalize(x, dim=-1, p=2, eps=1e-5) if normalize else x
    m = w.sum(-1) != 0
    s = w.sum(1) / m.sum(1).unsqueeze(-1)
    if normalize:
        s = F.normalize(s, dim=-1, p=2, eps=1e-5)
    return w, m, s


def weighted_sum(vals, weights, dt=F64):
    """criterion.py:361-365: the slots of weight 0 are logged values outside the total (they may be non-finite)"""
    keep = weights != 0
    return (vals.to(dt)[keep] * weights.to(dt)[keep]).sum()


# ------------------------------------------------------------------------------------------------------- error bounds
# First-order worst-case bounds of a float32 evaluation in units of U = U32, computed from the inputs and the fp64
# intermediates only.  A sum of n terms is charged (n - 1) U of the sum of magnitudes whatever its order (serial, wave
# butterflies, atomics); every other operation U of its result.  The intrinsics:
#   __expf(x)   relative (1.5 |x| + 2) U, the figure of tests/attn_ref.py; with the rounding of its argument x = a - b
#               (U |x| absolute, i.e. U |x| relative in the result)            EXPF(x) = 2.5 |x| + 2, and 0 at x = 0
#   __logf(y)   = v_log_f32(y) x ln 2.  The CDNA3/CDNA4 ISA guides give V_LOG_F32 1 ULP = 2 U relative of log2 y; the
#               product with the rounded constant ln 2 adds 2 U: 4 U |ln y| absolute.  Near y = 1 a relative figure of
#               the result is not promised, so an absolute floor of 4 U is charged as well  LOGF(y) = 4 |ln y| + 4
#               (the one-ULP library expf / logf of the set-loss and rec_ss kernels are inside both figures).
# An element (or row) of a gradient is held to  U x [bound + K 2^-12 R_max]: the bound is built from the magnitudes its
# own terms can reach (R, not the result, so cancellation is paid for), and the floor -- R_max the largest such magnitude
# of the tensor -- only guards entries whose terms underflow.  Where a kernel must write an exact zero the bound is 0, and
# `excess` then asks for equality.


def EXPF(x):
    return (2.5 * x.abs() + 2.0) * (x != 0)  # (exp(0) = 1 exactly)


def LOGF(y):
    return 4.0 * torch.log(y).abs() + 4.0


def _floor(b, R, K, dim=None):
    """dim: the floor's R_max is taken along that axis alone (rows whose scales differ by construction)"""
    return U32 * (b + K * FLOOR * (R.max() if dim is None else R.amax(dim, keepdim=True)))


def nll_bounds(logit, label, row_grad=None, eps=0.1, kg=0.0):
    """-> dict(lse (R), row_loss (R)[, dlogit (R, C)]).  Row r, d_c = x_c - max, E = sum_c exp(d_c) in [1, C]:
    E      each term EXPF(d_c), the sum (C - 1)                     -> relative  kE = sum_c e_c EXPF(d_c) / E + C - 1
    lse    = max + log E: kE + LOGF(E) + the sum's rounding          -> B_lse = kE + LOGF(E) + |lse|
    nll    = lse - x_label                                           -> B_lse + |nll|
    smooth = C lse - sum x: C B_lse + C |lse| + (C - 1) sum|x| + |smooth|
    loss   = (1 - eps) nll + eps / C smooth: (1 - eps) (B_lse + 3 |nll|) + eps / C (B_smooth + 3 |smooth|) + |loss|  (the
             difference, the factor and the product of each term, the final sum)
    dlogit_c = g (p_c - (1 - eps)[c = label] - eps / C), p_c = exp(x_c - lse): EXPF(x_c - lse) + B_lse relative in p_c,
    two subtractions and the product 3 U of the terms' magnitudes R_c = |g| (p_c + (1 - eps)[c = label] + eps / C); kg: the
    relative error of the row weights g themselves, in U."""
    x = logit.double()
    C = x.shape[1]
    d = x - x.amax(1, keepdim=True)
    e = torch.exp(d)
    E = e.sum(1)
    lse = torch.logsumexp(x, 1)
    kE = (e * EXPF(d)).sum(1) / E + (C - 1)
    B_lse = kE + LOGF(E) + lse.abs()
    nll = lse - x.gather(1, label[:, None]).squeeze(1)
    smooth = C * lse - x.sum(1)
    loss = (1 - eps) * nll + eps / C * smooth
    B_sm = C * B_lse + C * lse.abs() + (C - 1) * x.abs().sum(1) + smooth.abs()
    B_loss = (1 - eps) * (B_lse + 3 * nll.abs()) + eps / C * (B_sm + 3 * smooth.abs()) + loss.abs()
    out = {"lse": U32 * B_lse, "row_loss": U32 * B_loss}
    if row_grad is not None:
        g = row_grad.double().abs()[:, None]
        p = torch.exp(x - lse[:, None])
        oh = torch.zeros_like(x).scatter_(1, label[:, None], 1.0)
        R = g * (p + (1 - eps) * oh + eps / C)
        b = g * p * (EXPF(x - lse[:, None]) + B_lse[:, None]) + (3 + kg) * R
        out["dlogit"] = _floor(b, R, float(B_lse.max()) + 8) * (g > 0)  # (a masked row: exactly zero)
    return out


def rec_fw_bounds(row_loss, mask, g=None):
    """loss: a sum of Lw terms and a quotient per pair, a sum of N terms and a quotient: (N + Lw + 2) U of the mean of the
    magnitudes; accuracy: exact counts below 2^24 and one quotient: 2 U; row weights g / (N cnt): 3 U each."""
    m = mask.double()
    N, Lw = m.shape
    mag = ((row_loss.double().abs() * m).sum(1) / m.sum(1)).mean()
    out = {"loss": U32 * (N + Lw + 2) * mag, "acc": 2 * U32}
    if g is not None:
        out["rowgrad"] = 3 * U32 * abs(float(g)) / (N * m.sum(1, keepdim=True)) * m
    return out


def rowdot_bounds(a, b, scale, ds=None):
    """s: D products, D - 1 additions, the scale: (D + 1) U scale sum_d |a_d b_d|; da = ds b scale: 2 U |da|;
    db = scale sum_l ds a over the non-zero ds: (their number + 1) U scale sum_l |ds a|."""
    a, b = a.double().abs(), b.double().abs()
    N, L, D = a.shape
    out = {"s": U32 * (D + 1) * abs(scale) * (a * b.unsqueeze(1)).sum(-1)}
    if ds is not None:
        ds = ds.double().abs()
        out["da"] = 2 * U32 * abs(scale) * ds.unsqueeze(-1) * b.unsqueeze(1)
        nz = (ds != 0).sum(1, keepdim=True).double()  # (a zero weight adds an exact zero)
        out["db"] = U32 * (nz + 1) * abs(scale) * (ds.unsqueeze(-1) * a).sum(1)
    return out


def _normalize_bounds(v, dv, eps):
    """y = v / max(|v|, eps) along the last axis given the absolute error dv of v (units of U, first order): the norm --
    D squares, D - 1 additions, a root -- carries (D / 2 + 1) relative and |dv|_2 / |v| from its operand, the clamp or
    reciprocal and the product 3 more (D = the non-zero entries)
    -> dy_c <= dv_c / n + |y_c| (|dv|_2 / n + D / 2 + 4), n = max(|v|, eps)."""
    D = (v != 0).sum(-1, keepdim=True).to(v.dtype)  # (a zero term adds no rounding error)
    n = v.norm(dim=-1, keepdim=True).clamp(min=eps)
    return dv / n + (v / n).abs() * (dv.norm(dim=-1, keepdim=True) / n + D / 2 + 4)


def text_prep_bounds(x, normalize=True):
    """words: _normalize_bounds of exact inputs (0 when normalize is off); sentence: the mean over Lw words -- their own
    errors, Lw - 1 additions and the quotient -- then _normalize_bounds again.  -> dict(words (N, Lw, D), sent (N, D))"""
    x = x.double()
    N, Lw, D = x.shape
    w, m, _ = text_prep(x, normalize)
    dw = _normalize_bounds(x, torch.zeros_like(x), 1e-5) if normalize else torch.zeros_like(x)
    cnt = m.sum(1).unsqueeze(-1).double()
    mean = w.sum(1) / cnt
    dmean = (dw.sum(1) + (Lw + 1) * w.abs().sum(1)) / cnt
    ds = _normalize_bounds(mean, dmean, 1e-5) if normalize else dmean
    return {"words": U32 * dw, "sent": U32 * ds}


def weighted_sum_bounds(vals, weights):
    keep = weights != 0
    return U32 * (int(keep.sum()) + 1) * (vals.double()[keep] * weights.double()[keep]).abs().sum()


def saliency_bounds(s_pos, s_neg, label, vmask, pos_idx, neg_idx, rank_coef, margin, gscale=None):
    """-> dict(loss[, ds_pos (N, L), ds_neg (N, L)]).  Pair n, its 2L elements x_j = (v s + (1 - v)(-1e3)) / 0.5 (exact in
    float32: one addend is zero, the divisor a power of two), d_j = x_j - max, e_j = exp(d_j), T = sum e_j + 1e-6:
    T      relative kT = sum_j e_j EXPF(d_j) / T + 2 L        (2L - 1 additions and the constant)
    lp_j   = d_j - log T: B_lp_j = kT + LOGF(T) + 2 |lp_j|
    w_j    = v sum_{r <= stage_j} i_r, i_r = 1 / (cnt_r + 1e-6): a sum and a reciprocal (2 U of i_r) and stage_j - 1
             additions: kw_j = stage_j + 1
    rank_n = - sum_j w_j lp_j: sum_j w_j (B_lp_j + (kw_j + 2 L) |lp_j|)
    neg_n  = sum_l v -log(1 - sigmoid(s)): sigmoid relative (1.5 |s| + 4) (its __expf, a sum, a reciprocal); 1 - sigmoid
             carries that times sigmoid / (1 - sigmoid) = e^s -- the condition number 1 / (1 - sigmoid(s)) of the term --
             plus its own rounding, the log LOGF: B_l = e^s (1.5 |s| + 4) + 1 + LOGF(1 - sigmoid) and L |term| for the sum
    trip_n = sum_c max(0, margin + s_neg_c - s_pos_c): the float32 margin, two additions: 3 (|margin| + |s_n| + |s_p|) each
    loss   = sum_n [rank_n / (N rank_coef) + neg_n / N + 2 trip_n / (N P)]: the pairs' bounds with the same factors and
             (N + 6) U of the sum of magnitudes.
    gradient of element j: gs [2 v dx_j / (N rank_coef) + (neg half) v sigmoid / N  +- (pos half) 2 / (N P) per live
    triplet], dx_j = -(w_j - wsum s_j), s_j = q_j + [j = argmax] 1e-6 / T, q_j = e_j / T relative EXPF(d_j) + kT + 1.  w_j and
    wsum are sums of the same float32 values i_r, dx_j = - sum_r i_r (v_j [j in r] - cnt_r s_j), so the 2 U of each i_r are
    charged on |v_j [j in r] - cnt_r s_j|, which the fp64 intermediates give (0 where a row's only positive holds all the
    softmax mass), and only the additions on the magnitudes: stage_j - 1 of w_j, (max stage - 1) + (non-zero terms - 1) of
    wsum; the factors 1 / (N rank_coef), 2 / (N P), 1 / N and gs 4 U more."""
    sp, sn = s_pos.double(), s_neg.double()
    N, L = sp.shape
    vm = vmask.double()
    vm2 = vm.repeat(1, 2)
    lab = torch.cat([label.double(), torch.zeros_like(label.double())], 1)
    x = (vm2 * torch.cat([sp, sn], 1) + (1 - vm2) * -1e3) / 0.5
    mx, am = first_max(x)
    d = x - mx
    e = torch.exp(d)
    T = e.sum(1, keepdim=True) + 1e-6
    kT = (e * EXPF(d)).sum(1, keepdim=True) / T + 2 * L
    lp = d - torch.log(T)
    B_lp = kT + LOGF(T) + 2 * lp.abs()
    w = torch.zeros_like(x)
    stages = []  # (i_r, v_j [j in r], cnt_r) of the stages that some clip of the pair reaches
    for r in range(1, 12):
        pos = (lab >= r).double()
        c = pos.sum(1, keepdim=True)
        inv = torch.where(c > 0, 1 / (c + 1e-6), torch.zeros_like(c))
        w = w + inv * pos * vm2
        stages.append((inv, pos * vm2, (pos * vm2).sum(1, keepdim=True)))
    kw = lab.clamp(max=11) + 1
    B_rank = (w * (B_lp + (kw + 2 * L) * lp.abs())).sum(1)
    sg = torch.sigmoid(sn)
    term = -torch.log(1 - sg) * vm
    B_sg = 1.5 * sn.abs() + 4
    B_neg = (vm * (torch.exp(sn) * B_sg + 1 + LOGF(1 - sg)) + L * term).sum(1)
    mag = (w * lp.abs()).sum(1) / (N * rank_coef) + term.sum(1) / N
    b = B_rank / (N * rank_coef) + B_neg / N
    P = 0
    if pos_idx is not None:
        P = pos_idx.shape[1]
        ps, ns = sp.gather(1, pos_idx), sp.gather(1, neg_idx)
        t = margin + ns - ps
        b = b + 2 * (3 * (abs(margin) + ns.abs() + ps.abs()) * (t > -1e-3)).sum(1) / (N * P)
        mag = mag + 2 * t.clamp(min=0).sum(1) / (N * P)
    out = {"loss": U32 * (b.sum() + (N + 6) * mag.sum())}
    if gscale is None:
        return out
    gs = abs(float(gscale))
    wsum = w.sum(1, keepdim=True)
    ka = (kw - 2).clamp(min=0)  # the additions of w_j
    kws = ka.amax(1, keepdim=True) + ((w > 0).sum(1, keepdim=True) - 1).clamp(min=0)
    q = e / T
    a = torch.zeros_like(x).scatter_(1, am, 1.0) * 1e-6 / T
    b_inv = sum(2 * inv * (pj - cr * (q + a)).abs() for inv, pj, cr in stages)
    kr = 2.0 * vm2 / (N * rank_coef)
    R = kr * (w + wsum * (q + a))
    bb = kr * (b_inv + w * (ka + 5) + wsum * q * (kws + EXPF(d) + kT + 6) + wsum * a * (kws + kT + 6))
    Rp, Rn, bp, bn = R[:, :L].clone(), R[:, L:].clone(), bb[:, :L].clone(), bb[:, L:].clone()
    Rn += vm * sg / N
    bn += vm * sg / N * (B_sg + 3)
    if pos_idx is not None:
        live = (t >= 0).double() * 2.0 / (N * P)
        cnt = torch.zeros_like(sp).scatter_add_(1, pos_idx, live).add_(torch.zeros_like(sp).scatter_add_(1, neg_idx, live))
        Rp += cnt
        bp += cnt * (P + 5)
    K = float((kws + kT).max()) + 40.0
    # (a padded clip that no live triplet touches: exactly zero)
    out["ds_pos"] = _floor(gs * bp, gs * torch.cat([Rp, Rn]), K) * (Rp > 0)
    out["ds_neg"] = _floor(gs * bn, gs * torch.cat([Rp, Rn]), K) * (vm > 0)
    return out


def _giou_parts(src, tx):
    """matched rows: src (M, 2) as (cx, w), tx (M, 2) as (start, end) -> fp64 parts and their float32 error bounds in U:
    x1, x2 = cx -+ w / 2 carry e = |cx| + |w| each; raw_i = min - max: 2 e + |raw_i|; union = (x2 - x1) + (g2 - g1) - inter:
    its operands' errors and 3 roundings of the magnitudes; enc likewise."""
    cx, w = src[:, 0], src[:, 1]
    x1, x2, g1, g2 = cx - 0.5 * w, cx + 0.5 * w, tx[:, 0], tx[:, 1]
    e = cx.abs() + w.abs()
    raw_i = torch.min(x2, g2) - torch.max(x1, g1)
    inter = raw_i.clamp(min=0)
    uni = (x2 - x1) + (g2 - g1) - inter
    enc = (torch.max(x2, g2) - torch.min(x1, g1)).clamp(min=0)
    d_i = 2 * e + raw_i.abs()
    d_u = 2 * e + d_i + 3 * ((x2 - x1).abs() + (g2 - g1).abs() + inter)
    d_e = 2 * e + enc
    return inter, uni, enc, d_i, d_u, d_e


def set_loss_bounds(logits, spans, tgt_cxw, tgt_xx, tgt_off, match_q, eos_coef, g3=None):
    """-> dict(out4 (4)[, dlogits (N, Q, 2), dspans (N, Q, 2)]) with nm matched pairs:
    loss_span   2 nm differences (their operands exact), the sum, the quotient: (2 nm + 3) U loss_span
    loss_giou   1 - I/U + (E - U)/E per pair from _giou_parts: d_i / U + I d_u / U^2 + d_u / E + U d_e / E^2 + 6 (their
                magnitudes), then the sum and the quotient (nm + 2) U of the mean of 2 + |giou|
    loss_label  lse = max + log(e0 + e1): EXPF(l0 - l1) + 1 + LOGF(2) + |lse|, then - (l - lse) w: + 3 |ce|; the mean N Q + 2
    class_error exact comparisons and counts, 100 - ok (100 / nm): the quotient and the product 2 U of ok 100 / nm, the
                difference U of the result
    dlogits     gl (p_c - [c = cls]), gl = g w / (N Q): p_c relative EXPF(l0 - l1) + 3, 5 U of |gl| (p_c + [c = cls])
    dspans      L1: +- g / (2 nm): 4 U; gIoU: -(dI U - I dU) / U^2 - (dU E - U dE) / E^2 with the tie weights dI, dU, dE exact
                in [-1, 1]: (d_u + d_i) / U^2 + (U + I) / U^2 (2 d_u / U + 5) + (d_u + d_e) / E^2 + (E + U) / E^2 (2 d_e / E + 5),
                for both ends, and 6 U of the magnitudes for the sums and g / nm."""
    N, Q = logits.shape[:2]
    T = int(tgt_off[-1])
    flat, keep = matched(tgt_off, match_q, Q)
    nm = flat.numel()
    src = spans.double().reshape(-1, 2)[flat]
    tc, tx = tgt_cxw[:T].double()[keep], tgt_xx[:T].double()[keep]
    l1 = (src - tc).abs().sum() / (2 * nm)
    inter, uni, enc, d_i, d_u, d_e = _giou_parts(src, tx)
    Lg = 1 - (inter / uni - (enc - uni) / enc)
    b_g = d_i / uni + inter * d_u / uni ** 2 + d_u / enc + uni * d_e / enc ** 2 + 6 * (inter / uni + uni / enc + 2)
    lg = logits.double().reshape(N * Q, 2)
    dl = (lg[:, 0] - lg[:, 1]).abs()
    lse = torch.logsumexp(lg, 1)
    cls = torch.ones(N * Q, dtype=torch.int64, device=logits.device)
    cls[flat] = 0
    wq = torch.where(cls == 0, 1.0, eos_coef)
    ce = (lse - lg.gather(1, cls[:, None]).squeeze(1)) * wq
    b_ce = wq * (EXPF(dl) + 1 + LOGF(torch.tensor(2.0)) + lse.abs()) + 3 * ce
    picked = lg[flat]
    okf = (picked[:, 0] >= picked[:, 1]).double().sum() * (100.0 / nm)
    out4 = torch.stack([(2 * nm + 3) * l1, b_g.sum() / nm + (nm + 2) * (2 + Lg.abs()).mean(),
                        b_ce.mean() + (N * Q + 2) * ce.mean(), 2 * okf + (100 - okf).abs()])
    out = {"out4": U32 * out4}
    if g3 is None:
        return out
    g = g3.double().abs()
    gl = (g[2] * wq / (N * Q))[:, None]
    p = torch.softmax(lg, 1)
    oh = torch.zeros_like(lg).scatter_(1, cls[:, None], 1.0)
    R = gl * (p + oh)
    out["dlogits"] = _floor(gl * p * (EXPF(dl)[:, None] + 3) + 5 * R, R, float(EXPF(dl).max()) + 8).reshape(N, Q, 2)
    Mg = (uni + inter) / uni ** 2 + (enc + uni) / enc ** 2
    eg = ((d_u + d_i) / uni ** 2 + (uni + inter) / uni ** 2 * (2 * d_u / uni + 5)
          + (d_u + d_e) / enc ** 2 + (enc + uni) / enc ** 2 * (2 * d_e / enc + 5))
    Rm = g[0] / (2 * nm) + g[1] / nm * 2 * Mg
    bm = 4 * g[0] / (2 * nm) + g[1] / nm * (2 * eg + 12 * Mg)
    Rs = torch.zeros(N * Q, dtype=F64, device=logits.device).index_put_((flat,), Rm)
    bs = torch.zeros(N * Q, dtype=F64, device=logits.device).index_put_((flat,), bm)
    K = float((eg / Mg.clamp(min=1e-300)).max()) + 16 if nm else 16.0
    out["dspans"] = (_floor(bs, Rs, K) * (Rs > 0))[:, None].expand(N * Q, 2).reshape(N, Q, 2)  # (unmatched query: zero)
    return out


def rec_ss_bounds(pv, cmask, ew, wmask, pos, tau, g=None):
    """-> dict(cn, wn (N, D), sim (N, N), rows (N), loss[, dpv (N, D), dew (N, D): per pair and column, every valid clip /
    word row of the pair carries the same values]).
    mean    clip_c = sum_l m pv / cnt over the cnt valid rows (a masked row adds an exact zero): the last addition of any
            summation tree rounds the result itself, the cnt - 2 before it at most the magnitudes' sum, then the quotient:
            [(cnt - 2) sum_l m |pv_c| + 2 |sum|] / cnt  (two rows v, -v: exactly 0)
    cn, wn  _normalize_bounds(mean, its error, 1e-12)
    sim_nk  = <cn_n, wn_k> / tau: sum_c (dcn |wn| + |cn| dwn) + (D + 3) sum_c |cn wn|, over tau
    row_n   lg_k = sim_k - max: the maximum is one of the row's own float32 values and cancels between lg_k and log S, so
            dlg_k = dsim_k + |lg_k| (exactly 0 at the argmax); S = sum_k exp(lg_k): sum_k e_k (EXPF(lg_k) + dlg_k / U)
            + (N - 1) S; log(S + 1e-6): LOGF + dS / S; logp_k: dlg_k + dlogS + |logp_k|; the positives' sum and the quotient
            (cnt + 3) U of the magnitudes
    loss    the rows' mean: (N + 1) U more
    dsim_nk = a_n (-pos_k + cnt (e_k + [k = argmax] 1e-6) / S'), S' = S + 1e-6, a_n = g / (N (cnt + 1e-6) tau).  a_n is one
            float32 value, a common factor: its roundings (g, / N, cnt + 1e-6, the quotient, 1 / tau and that product) and
            the two additions are relative to the result, 8 U |dsim_nk|; -a pos is exact; a cnt e_k / S' carries
            EXPF(lg_k) + dlg_k + kS and 5 roundings (S', its reciprocal, three products) of a cnt p_k, the correction kS + 6 of
            a cnt 1e-6 / S'.  (One pair alone: S = 1 exactly, dsim = 0, and the bound is 5 U of a.)
    dcn_n   = sum_k dsim_nk wn_k: the operands' errors, and N products and N - 1 additions of the actual terms: N U of
            R = sum_k |dsim_nk| |wn_k| -- the cancellation inside dsim_nk is paid above, the sum over k here; the projection
            dcn - cn (cn . dcn): the dot product's (D + 1) U of sum_c |cn_c| R_c, both operands' errors, 5 U of R + |cn| (|cn| . R)
            for the difference and the scale 1 / (norm cnt) (dew alike from dsim^T, cn)."""
    pv, ew = pv.double(), ew.double()
    N, Lv, D = pv.shape
    cm, wm = cmask.double().unsqueeze(-1), wmask.double().unsqueeze(-1)
    ref = rec_ss(pv, cmask, ew, wmask, pos, tau)
    out = {}
    norm, dn = {}, {}
    for name, xx, mm in (("cn", pv, cm), ("wn", ew, wm)):
        cnt = mm.sum(1)
        mean = (xx * mm).sum(1) / cnt
        dm = ((cnt - 2).clamp(min=0) * (xx.abs() * mm).sum(1) + 2 * (xx * mm).sum(1).abs()) / cnt
        dn[name] = _normalize_bounds(mean, dm, 1e-12)
        norm[name] = mean.norm(dim=-1, keepdim=True).clamp(min=1e-12) * cnt
        out[name] = U32 * dn[name]
    cn, wn = ref["cn"].abs(), ref["wn"].abs()
    D = int(((cn != 0).any(0) & (wn != 0).any(0)).sum())  # (the columns whose products are not exact zeros)
    dsim = (dn["cn"] @ wn.t() + cn @ dn["wn"].t() + (D + 3) * (cn @ wn.t())) / tau
    out["sim"] = U32 * dsim
    sim = ref["sim"]
    mx, am = first_max(sim)
    lg = sim - mx
    dlg = (dsim + lg.abs()).scatter(1, am, 0.0)
    e = torch.exp(lg)
    S = e.sum(1, keepdim=True)
    kS = (e * (EXPF(lg) + dlg)).sum(1, keepdim=True) / S + (N - 1)
    logp = lg - torch.log(S + 1e-6)
    dlogp = dlg + kS + LOGF(S + 1e-6) + logp.abs()
    p = pos.double()
    cnt = p.sum(1)
    out["rows"] = U32 * ((p * dlogp).sum(1) + (cnt + 3) * (p * logp.abs()).sum(1)) / (cnt + 1e-6)
    out["loss"] = out["rows"].sum() / N + U32 * (N + 1) * ref["rows"].abs().sum() / N
    if g is None:
        return out
    a = (abs(float(g)) / (N * (cnt + 1e-6)))[:, None] / tau
    pk = e / (S + 1e-6)
    corr = torch.zeros_like(sim).scatter_(1, am, 1.0) * 1e-6 / (S + 1e-6)
    c1 = cnt[:, None]
    Dm = (a * (-p + c1 * (pk + corr))).abs()
    dA = a * c1 * pk * (EXPF(lg) + dlg + kS + 5) + a * c1 * corr * (kS + 6) + 8 * Dm
    for name, DD, dAA, own, oth in (("dpv", Dm, dA, "cn", "wn"), ("dew", Dm.t(), dA.t(), "wn", "cn")):
        y, dy = ref[own].abs(), dn[own]
        Rg = DD @ ref[oth].abs()
        dg = dAA @ ref[oth].abs() + DD @ dn[oth] + N * Rg
        dot = (y * Rg).sum(1, keepdim=True)
        ddot = (y * dg + dy * Rg).sum(1, keepdim=True) + (D + 1) * dot
        Rt = Rg + y * dot
        bt = dg + y * ddot + dy * dot + 5 * Rt
        K = float((bt / Rt.clamp(min=1e-300))[Rt > 0].max()) if bool((Rt > 0).any()) else 0.0
        out[name] = _floor(bt / norm[own], Rt / norm[own], K, dim=1)  # (per pair: the clamp branch scales a pair's rows by 1e12)
    return out


# ------------------------------------------------------------------------------------------------------- block drivers
# One case of tests/loss_cases.py -> every output a kernel form produces, as the reference states it (out_*) and as far as a
# float32 evaluation may be from it (bnd_*, same keys); n_valid = k: the first k pairs alone, zeros (held exactly) beyond.
G_SAL, G_SS, G_FW = 0.7, 0.9, 0.7   # upstream gradients
G_SET = (0.7, -1.3, 2.1)


def _pad0(t, N):
    """t (k, ...) -> (N, ...) with zero rows beyond"""
    out = torch.zeros((N,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    out[:t.shape[0]] = t
    return out


def _leaf(t, dt):
    return t.detach().to(dt).clone().requires_grad_()


def excess(got, ref, bound):
    """largest |got - ref| in units of the bound (0 where both are 0: an exact zero is held exactly)"""
    err = (got.double() - ref.double()).abs()
    bound = bound.double().expand_as(err)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(torch.nan_to_num(r, nan=float("inf")).max()) if r.numel() else 0.0


def _nll_mask(c):
    R = c["logit"].shape[0]
    m = c["mask"] if c["mask"] is not None else torch.ones(R, dtype=torch.bool, device=c["logit"].device)
    return m.view(c["N"], c["Lw"])


def out_nll(c, nv=None, dt=F64):
    N, Lw = c["N"], c["Lw"]
    m = _nll_mask(c)
    row_loss, lse, correct = nll_smooth(c["logit"], c["label"], c["mask"], c["eps"], dt)
    loss, acc = rec_fw_reduce(row_loss.view(N, Lw), correct.view(N, Lw), m, nv, dt)
    rg = rec_fw_rowgrad(m, G_FW, nv, dt).reshape(-1)
    return dict(row_loss=row_loss, lse=lse, correct=correct.to(dt), fw_loss=loss, fw_acc=acc, rowgrad=rg,
                dlogit=nll_grad(c["logit"], c["label"], lse, rg, c["eps"], dt))


def bnd_nll(c, nv=None):
    N, Lw = c["N"], c["Lw"]
    k = N if nv is None else nv
    m = _nll_mask(c)
    ref = out_nll(c, nv)
    b = nll_bounds(c["logit"], c["label"], ref["rowgrad"], c["eps"], kg=3.0)
    fb = rec_fw_bounds(ref["row_loss"].view(N, Lw)[:k], m[:k], G_FW)
    md = m.double()
    rows = (b["row_loss"].view(N, Lw) * md)[:k].sum(1) / md[:k].sum(1)
    zero = torch.zeros((), dtype=F64, device=m.device)
    return dict(row_loss=b["row_loss"] * md.reshape(-1), lse=b["lse"], correct=zero, fw_loss=fb["loss"] + rows.sum() / k,
                fw_acc=zero + fb["acc"], rowgrad=_pad0(fb["rowgrad"], N).reshape(-1), dlogit=b["dlogit"])


def out_fw(c, nv=None, dt=F64):
    loss, acc = rec_fw_reduce(c["row_loss"], c["correct"], c["mask"], nv, dt)
    return dict(fw_loss=loss, fw_acc=acc, rowgrad=rec_fw_rowgrad(c["mask"], G_FW, nv, dt))


def bnd_fw(c, nv=None):
    N = c["mask"].shape[0]
    k = N if nv is None else nv
    fb = rec_fw_bounds(c["row_loss"][:k], c["mask"][:k], G_FW)
    return dict(fw_loss=fb["loss"], fw_acc=torch.zeros((), dtype=F64) + fb["acc"], rowgrad=_pad0(fb["rowgrad"], N))


_SAL_KEYS = ("s_pos", "s_neg", "label", "vmask", "pos_idx", "neg_idx")


def out_sal(c, nv=None, dt=F64):
    sp, sn = _leaf(c["s_pos"], dt), _leaf(c["s_neg"], dt)
    loss = saliency(sp, sn, c["label"], c["vmask"], c["pos_idx"], c["neg_idx"], c["rank_coef"], c["margin"], nv, dt)
    gp, gn = torch.autograd.grad(loss, (sp, sn))
    return dict(loss=loss.detach(), ds_pos=G_SAL * gp, ds_neg=G_SAL * gn)


def bnd_sal(c, nv=None):
    N = c["s_pos"].shape[0]
    k = N if nv is None else nv
    b = saliency_bounds(*lead(k, *[c[n] for n in _SAL_KEYS]), c["rank_coef"], c["margin"], G_SAL)
    return dict(loss=b["loss"], ds_pos=_pad0(b["ds_pos"], N), ds_neg=_pad0(b["ds_neg"], N))


def out_set(c, layer, match_q, nv=None, dt=F64):
    lg, sp = _leaf(c["logits"][layer], dt), _leaf(c["spans"][layer], dt)
    ls = set_losses(lg, sp, c["tgt_cxw"], c["tgt_xx"], c["tgt_off"], match_q, c["eos_coef"], nv, dt)
    dl, ds = torch.autograd.grad(G_SET[0] * ls[0] + G_SET[1] * ls[1] + G_SET[2] * ls[2], (lg, sp))
    return dict(out4=torch.stack([x.detach() for x in ls]), dlogits=dl, dspans=ds)


def bnd_set(c, layer, match_q, nv=None):
    N = c["logits"][layer].shape[0]
    k = N if nv is None else nv
    g3 = torch.tensor(G_SET, dtype=F64, device=c["tgt_off"].device)
    b = set_loss_bounds(c["logits"][layer][:k], c["spans"][layer][:k], c["tgt_cxw"], c["tgt_xx"], c["tgt_off"][:k + 1], match_q,
                        c["eos_coef"], g3)
    return dict(out4=b["out4"], dlogits=_pad0(b["dlogits"], N), dspans=_pad0(b["dspans"], N))


def out_ss(c, nv=None, dt=F64):
    """cn, wn: every pair of the capacity (the masked means do not depend on the count); sim (k, k), rows (k)"""
    pv, ew = _leaf(c["pv"], dt), _leaf(c["ew"], dt)
    r = rec_ss(pv, c["cmask"], ew, c["wmask"], c["pos"], c["tau"], nv, dt)
    dpv, dew = torch.autograd.grad(r["loss"], (pv, ew))
    full = r if nv is None else rec_ss(pv, c["cmask"], ew, c["wmask"], c["pos"], c["tau"], None, dt)
    return dict(loss=r["loss"].detach(), cn=full["cn"].detach(), wn=full["wn"].detach(), sim=r["sim"].detach(),
                rows=r["rows"].detach(), dpv=G_SS * dpv, dew=G_SS * dew)


def bnd_ss(c, nv=None):
    N = c["pv"].shape[0]
    k = N if nv is None else nv
    b = rec_ss_bounds(c["pv"][:k], c["cmask"][:k], c["ew"][:k], c["wmask"][:k], c["pos"][:k, :k], c["tau"], G_SS)
    full = b if nv is None else rec_ss_bounds(c["pv"], c["cmask"], c["ew"], c["wmask"], c["pos"], c["tau"])
    return dict(loss=b["loss"], cn=full["cn"], wn=full["wn"], sim=b["sim"], rows=b["rows"],
                dpv=_pad0(b["dpv"], N).unsqueeze(1) * c["cmask"].double().unsqueeze(-1),   # (a masked clip: exactly zero)
                dew=_pad0(b["dew"], N).unsqueeze(1) * c["wmask"].double().unsqueeze(-1))
