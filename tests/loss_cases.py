"""The named cases of tests/test_loss_kernels_gpu.py, built on the CPU; tests/test_loss_ref_cpu.py checks on every one of
them that a float32 evaluation of the reference stays inside the derived bounds of tests/loss_ref.py and that the bounds
stay under the suite's older whole-tensor 1e-4.  A case that failed either condition was re-chosen, never the bound:
  * an order-free bound charges a sum of n non-zero terms (n - 1) U of their magnitudes, so long sums of terms of either
    sign (a dense D = 1024 dot product over tau = 0.07, a masked mean of 1030 clips, 600 weighted rows) are ill-conditioned
    next to a result of order 1.  Those extents keep their shape and reach the same code, with few non-zero terms: features
    on every 16th column and the last one, few valid clips, few weighted rows (exact zeros add no rounding error);
  * features that are means of random vectors cancel: clip, word and text features carry a per-pair offset.
Every builder returns CPU tensors; `nv` lists the device counts 0 < n_valid < N to run besides n_valid = N."""
import torch


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------ NLL
def nll_case(C, seed, shift=0.0, tie=False, last=False, one=False, nomask=False, N=3, Lw=3):
    g = _g(seed)
    R = N * Lw
    logit = torch.randn(R, C, generator=g) + shift
    label = torch.randint(0, C, (R,), generator=g)
    mask = torch.ones(R, dtype=torch.bool)
    mask[1] = mask[R - 1] = False
    if tie and C > 1:  # the row maximum occurs twice: the first index wins; it is the label in the even rows
        for r in range(R):
            a, b = sorted(torch.randperm(C, generator=g)[:2].tolist())
            logit[r, a] = logit[r, b] = logit[r].max() + 0.5
            label[r] = a if r % 2 == 0 else b
    if last:
        label[:] = C - 1
    if one:
        mask[:] = False
        mask[4] = True
    return dict(logit=logit, label=label, mask=None if nomask else mask, eps=0.1, N=N, Lw=Lw, nv=[2] if N > 2 else [])


NLL = {"C%d" % C: (lambda C=C: nll_case(C, 100 + C)) for C in (1, 2, 53, 2048, 2049, 5003, 5120, 5121, 6001)}
NLL.update({
    "shift100_C53": lambda: nll_case(53, 1, shift=100.0),  # total - C lse cancels
    "tie_C2049": lambda: nll_case(2049, 2, tie=True),
    "tie_C53": lambda: nll_case(53, 3, tie=True),
    "last_label_C5121": lambda: nll_case(5121, 4, last=True),
    "one_row_C53": lambda: nll_case(53, 5, one=True, N=1, Lw=9),
    "nomask_C2048": lambda: nll_case(2048, 6, nomask=True),
})


# ------------------------------------------------------------------------------------------------------------- saliency
def sal_case(N, L, seed, P=2, max_label=12, margin=0.2, rank_coef=12.0, dyadic=False, same_idx=False, all_pad=None,
             no_pos=None, keep=0.8):
    g = _g(seed)
    sp, sn = torch.randn(N, L, generator=g).clamp(-8, 8), torch.randn(N, L, generator=g).clamp(-8, 8)
    if dyadic:
        sp, sn = torch.round(sp * 64) / 64, torch.round(sn * 64) / 64
    vmask = torch.rand(N, L, generator=g) < keep
    vmask[:, 0] = True
    if all_pad is not None:
        vmask[all_pad] = False
    label = torch.randint(0, max_label + 1, (N, L), generator=g).double() * (torch.rand(N, L, generator=g) > 0.5)
    label = label * vmask
    if max_label == 12:
        label[N - 1, 0] = 12.0  # beyond the 11 stages
    if no_pos is not None:
        label[no_pos] = 0
    pos_idx = neg_idx = None
    if P:
        pos_idx, neg_idx = torch.randint(0, L, (N, P), generator=g), torch.randint(0, L, (N, P), generator=g)
        pos_idx[0, 0], neg_idx[N - 1, P - 1] = L - 1, L - 1  # the whole of L
        if same_idx:
            neg_idx[0, 0] = pos_idx[0, 0]
        if dyadic and L > 1:  # one triplet at the margin exactly: margin + s[neg] - s[pos] == 0 in float32 and float64
            pos_idx[N - 1, 0], neg_idx[N - 1, 0] = 0, 1
            sp[N - 1, 0] = sp[N - 1, 1] + margin
    return dict(s_pos=sp, s_neg=sn, label=label, vmask=vmask, pos_idx=pos_idx, neg_idx=neg_idx, rank_coef=rank_coef,
                margin=margin, nv=[] if N == 1 else [max(1, N // 2)])


SAL = {
    # one clip, one stage, no triplets, rank_coef 1: the argmax correction is the largest share of a gradient it can be
    "1x1": lambda: sal_case(1, 1, 10, P=0, max_label=1, rank_coef=1.0, keep=1.0),
    # pair 0: the positive clip far above the negative one -- the row's log-sum-exp is log(1 + 1e-6) and the positive's
    # gradient cancels to nothing but for the argmax correction; pair 1: two close scores far below 0, so that the softmax
    # share of the negative clip, which the + 1e-6 scales, is all of its gradient
    "2x1_far_near": lambda: dict(sal_case(2, 1, 10, P=0, max_label=1, rank_coef=1.0, keep=1.0), label=torch.ones(2, 1).double(), nv=[],
                                 s_pos=torch.tensor([[8.0], [-6.0]]), s_neg=torch.tensor([[-8.0], [-6.0625]])),
    "1x1_P1": lambda: sal_case(1, 1, 11, P=1, max_label=1, same_idx=True, keep=1.0),
    "5x64_label12_P2": lambda: sal_case(5, 64, 12, P=2, no_pos=0),
    "4x128_P64_allpad_stage3": lambda: sal_case(4, 128, 13, P=64, max_label=3, all_pad=2),  # stages 4..11: no pair
    "3x129_P1_same": lambda: sal_case(3, 129, 14, P=1, same_idx=True),
    "2x640_P2": lambda: sal_case(2, 640, 15, P=2),
    "17x75_margin_exact": lambda: sal_case(17, 75, 16, P=2, margin=0.25, dyadic=True, no_pos=3),
    "17x75_noP": lambda: sal_case(17, 75, 17, P=0, rank_coef=1.0),
}


# ----------------------------------------------------------------------------------------------------------- set losses
def _tgt(sizes, g):
    off = torch.tensor([0] + list(torch.tensor(sizes).cumsum(0)), dtype=torch.int32)
    T = int(off[-1])
    st = torch.rand(T, generator=g) * 0.6
    ed = st + 0.05 + torch.rand(T, generator=g) * 0.3
    return off, torch.stack([(st + ed) * 0.5, ed - st], 1), torch.stack([st, ed], 1)


def set_case(N, Q, tmax, seed, layers=1):
    g = _g(seed)
    sizes = [1 + (i % tmax) for i in range(N)]
    sizes[-1] = tmax
    off, cxw, xx = _tgt(sizes, g)
    logits = [torch.randn(N, Q, 2, generator=g) for _ in range(layers)]
    spans = [torch.sigmoid(torch.randn(N, Q, 2, generator=g)) for _ in range(layers)]
    for lg in logits:
        lg[0, :, 1] = lg[0, :, 0]  # l0 == l1: the first index is the argmax (class_error counts it as foreground)
    return dict(logits=logits, spans=spans, tgt_off=off, tgt_cxw=cxw, tgt_xx=xx, tmax=tmax, eos_coef=0.1,
                nv=[] if N == 1 else [max(1, N // 2)])


def set_tie_case():
    """seven pairs of one query and one target, every number dyadic (x1, x2 exact): right ends equal, left ends equal,
    touching (raw_i == 0), disjoint, identical, zero-width prediction in a wide target, cx == tc with w != tw"""
    pred = [(0.25, 0.75), (0.25, 0.5), (0.25, 0.5), (0.125, 0.25), (0.25, 0.75), (0.5, 0.5), (0.375, 0.625)]
    tgt = [(0.5, 0.75), (0.25, 0.75), (0.5, 0.75), (0.5, 0.625), (0.25, 0.75), (0.25, 0.75), (0.25, 0.75)]
    p, t = torch.tensor(pred), torch.tensor(tgt)
    spans = torch.stack([(p[:, 0] + p[:, 1]) / 2, p[:, 1] - p[:, 0]], 1).reshape(7, 1, 2)
    logits = torch.randn(7, 1, 2, generator=_g(7))
    logits[0, 0, 1] = logits[0, 0, 0]
    return dict(logits=[logits], spans=[spans], tgt_off=torch.arange(8, dtype=torch.int32),
                tgt_cxw=torch.stack([(t[:, 0] + t[:, 1]) / 2, t[:, 1] - t[:, 0]], 1), tgt_xx=t, tmax=1, eos_coef=0.1, nv=[3])


SET = {"%dx%dx%d" % s: (lambda s=s: set_case(*s, seed=200 + sum(s)))
       for s in ((1, 1, 1), (1, 64, 1), (3, 10, 10), (70, 12, 4), (5, 64, 64), (4, 3, 64), (33, 33, 2))}
SET["3x10x10_8layers"] = lambda: set_case(3, 10, 10, 230, layers=8)
SET["ties"] = set_tie_case


# --------------------------------------------------------------------------------------------------------------- rec_ss
def ss_case(N, Lv, Le, D, tau, seed, dense=False):
    g = _g(seed)
    cols = torch.ones(D, dtype=torch.bool)
    if D > 64 and not dense:  # (see the module docstring)
        cols[:] = False
        cols[::16] = True
        cols[D - 1] = True

    def feat(L):
        base = torch.randn(N, 1, D, generator=g)
        if dense:  # every column, lane and float4 component carries data; offsets of one sign keep the sums conditioned
            base = base.abs() + 0.5
        return (base + 0.25 * torch.randn(N, L, D, generator=g)) * cols

    pv, ew = feat(Lv), feat(Le)
    cmask = torch.rand(N, Lv, generator=g) < min(0.3, 10.0 / Lv)
    wmask = torch.rand(N, Le, generator=g) < min(0.7, 10.0 / Le)
    cmask[:, 0] = wmask[:, 0] = True
    cmask[:, Lv - 1] = wmask[:, Le - 1] = True
    pos = (torch.rand(N, N, generator=g) < 0.4) | torch.eye(N, dtype=torch.bool)
    if N > 1:
        pos[N - 1] = False          # a row without positives
        cmask[1] = False
        cmask[1, Lv // 2] = True    # a pair with one valid clip
    if N > 2 and Lv > 1:            # a pair whose masked clip mean is exactly zero: the clamp branch of the normalisation
        cmask[2] = False
        cmask[2, 0] = cmask[2, Lv - 1] = True
        pv[2, 0] = torch.round(pv[2, 0] * 64) / 64
        pv[2, Lv - 1] = -pv[2, 0]
        pos[2] = False              # (its similarities are all 0: with several positives its gradient would cancel)
        pos[2, 2] = True
    if N > 2 and Le > 1:            # and one whose masked word mean is exactly zero (the same branch on the words' side)
        k = 3 if N > 3 else 0
        wmask[k] = False
        wmask[k, 0] = wmask[k, Le - 1] = True
        ew[k, 0] = torch.round(ew[k, 0] * 64) / 64
        ew[k, Le - 1] = -ew[k, 0]
    return dict(pv=pv, cmask=cmask, ew=ew, wmask=wmask, pos=pos, tau=tau, nv=sorted({(N + 1) // 2, N - 1} - {0, N}))


SS_SEED = {(33, 7, 5, 64): 2, (70, 3, 2, 32): 2}  # (re-chosen: the first draw left dpv 2.1e-4 of its maximum)
SS = {"%dx%dx%dx%d_tau%s" % (s + (t,)): (lambda s=s, t=t: ss_case(*s, tau=t, seed=SS_SEED.get(s, 300 + sum(s))))
      for s, t in (((1, 1, 1, 4), 0.5), ((5, 20, 9, 30), 0.07), ((5, 20, 9, 33), 0.5), ((33, 7, 5, 64), 0.5),
                   ((70, 3, 2, 32), 0.5), ((4, 1030, 3, 8), 0.07), ((4, 6, 257, 8), 0.5), ((3, 5, 4, 1024), 0.07),
                   ((3, 5, 4, 260), 0.5))}
# every column of the D > 256 slices with data.  Forward only: means of one sign are nearly parallel, so the gradient through
# the normalisation cancels and is ill-conditioned (its bound is 6e-4 of it); the sparse 260 / 1024 cases hold the backward
SS["3x5x4x260_dense_tau0.5"] = lambda: dict(ss_case(3, 5, 4, 260, tau=0.5, seed=9, dense=True), skip=("dpv", "dew"))


# --------------------------------------------------------------------------------------------------- rec_fw reductions
def fw_case(N, Lw, seed):
    g = _g(seed)
    lens = torch.tensor([1 + (5 * i) % Lw for i in range(N)])  # pair 0: one valid word
    mask = torch.arange(Lw)[None] < lens[:, None]
    row_loss = (torch.rand(N, Lw, generator=g) * 9 + 0.5) * mask  # (zeros where masked, as nll_smooth_fwd leaves them)
    correct = (torch.rand(N, Lw, generator=g) < 0.4)
    return dict(row_loss=row_loss, correct=correct, mask=mask, nv=[] if N == 1 else [max(1, N // 2)])


FW = {"%dx%d" % s: (lambda s=s: fw_case(*s, seed=400 + sum(s))) for s in ((1, 1), (33, 7), (32, 32))}


# --------------------------------------------------------------------------------------------------------------- rowdot
def rowdot_case(N, L, D, seed):
    g = _g(seed)
    ds = torch.randn(N, L, generator=g)
    if L > 100:
        ds = ds * (torch.arange(L) % 13 == 0)  # (see the module docstring)
    b = torch.randn(N, D, generator=g)
    a = 0.5 * torch.randn(N, L, D, generator=g) + 0.5 * b.unsqueeze(1)  # (a dot product of independent signs cancels)
    return dict(a=a, b=b, ds=ds, scale=1.0 / 16.0)


ROWDOT = {"%dx%dx%d" % s: (lambda s=s: rowdot_case(*s, seed=500 + sum(s))) for s in ((1, 1, 4), (5, 75, 256), (3, 600, 32), (2, 9, 300))}


# ------------------------------------------------------------------------------------------------------------ text_prep
def text_case(N, Lw, D, seed):
    g = _g(seed)
    x = torch.randn(N, 1, D, generator=g) + 0.5 * torch.randn(N, Lw, D, generator=g)
    lens = torch.tensor([1 + (4 * i) % Lw for i in range(N)])  # pair 0: one valid word
    x = x * (torch.arange(Lw)[None] < lens[:, None]).unsqueeze(-1)
    if Lw >= 9:
        x[N - 1] = torch.randn(Lw, D, generator=g) + 1.0
        x[N - 1, 3] = x[N - 1, 3] * 1e-7        # a norm under the 1e-5 clamp, not zero
        x[N - 1, 5] = 0
        x[N - 1, 5, 0], x[N - 1, 5, 1] = 0.75, -0.75  # normalised sum exactly 0: masked out, features kept
    return dict(x=x)


TEXT = {"%dx%dx%d" % s: (lambda s=s: text_case(*s, seed=600 + sum(s))) for s in ((1, 1, 4), (5, 9, 300), (3, 32, 512), (2, 7, 768))}


# --------------------------------------------------------------------------------------------------------- weighted sum
def wsum_case(n, seed):
    g = _g(seed)
    v, w = torch.randn(n, generator=g).abs(), torch.rand(n, generator=g) + 0.1  # (loss values: positive)
    if n >= 13:
        v[3], v[7] = float("nan"), float("inf")  # logged-only slots
        w[3] = w[7] = 0.0
    return dict(vals=v, weights=w, g=2.5)


WSUM = {"n%d" % n: (lambda n=n: wsum_case(n, 700 + n)) for n in (1, 13, 256)}
