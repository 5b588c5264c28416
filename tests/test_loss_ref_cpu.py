"""The fp64 loss reference of tests/loss_ref.py, on the CPU:
  * every function reproduces oracle/mesm_oracle.py (float64 inputs, rtol = atol = 1e-12, values and autograd gradients) and
    tests/ref_losses.py evaluated in float64.  The oracle's generalized_temporal_iou casts to float32 itself
    (span_utils.py:103-104), so what passes through it is pinned twice: to the oracle's uncast temporal_iou and the
    enclosing-span formula at 1e-12, and to the cast function at float32 accuracy;
  * n_valid = k is the function on the sliced inputs, n_valid = N is None;
  * on every case of tests/loss_cases.py (the cases of tests/test_loss_kernels_gpu.py) a float32 evaluation of the reference
    -- loss_ref itself with dt = float32, and tests/ref_losses.py in float32 -- lies inside the derived bounds, and the
    bounds are at most the suite's older 1e-4 of the output's largest magnitude;
  * every seeded defect of a float32 copy of the reference falls outside the bounds on at least one case.

The older metric (largest absolute error over the largest magnitude of the whole tensor, < 1e-4, or 2e-4 for rec_ss'
gradients) lets four seeded defects through on runs where the bounds catch them (SLIP_THROUGH): the -eps / C term of the NLL
gradient at C = 2048, 2049 and 5003 (2e-5 of the row maximum at 5003), the + 1e-6 inside rec_ss' log and rec_ss' argmax
correction (4x1030x3x8, n_valid = 2), the saliency rows' argmax correction (2x1_far_near).  `>` for `>=` at the gIoU clamps
turns out unobservable (BENIGN).  The + 1e-6 inside a log is seeded in rec_ss; in the saliency rows it scales a softmax share
by 1e-6 / T, 17 U / T, and the order-free bound of that share is 12 U or more, so there it is not seeded."""
import contextlib

import pytest
import torch

import loss_cases as LC
import loss_ref as LR
import ref_losses as R
from oracle import mesm_oracle as mo

F32, F64 = torch.float32, torch.float64
TOL = dict(rtol=1e-12, atol=1e-12)
COST = dict(set_cost_span=10.0, set_cost_giou=1.0, set_cost_class=4.0)


def cpu_match(c, layer, k=None):
    """the reference's own matching (matcher.py:39-117 through the oracle and scipy) as match_q (sumT,) int32"""
    off = c["tgt_off"].tolist()
    N = c["logits"][layer].shape[0] if k is None else k
    T = off[N]
    targets = dict(norm_moment=[dict(moments=c["tgt_xx"][off[b]:off[b + 1]]) for b in range(N)],
                   norm_span=[dict(spans=c["tgt_cxw"][off[b]:off[b + 1]]) for b in range(N)])
    idx = mo.hungarian(c["logits"][layer][:N], c["spans"][layer][:N], targets, dict(COST, dataset_name="qvhighlights"))
    mq = torch.full((T,), -1, dtype=torch.int32)
    for b, (qi, ti) in enumerate(idx):
        mq[off[b] + ti] = qi.to(torch.int32)
    return mq


@contextlib.contextmanager
def oracle_in_float64():
    """the oracle adds Python floats to integer counts (`pos.sum(1) + 1e-6`), which gives a tensor of the default dtype:
    with float64 inputs it is evaluated in float64 throughout only under a float64 default"""
    torch.set_default_dtype(F64)
    try:
        yield
    finally:
        torch.set_default_dtype(F32)


def allclose(a, b):
    return torch.allclose(a.double(), b.double(), **TOL)  # (the oracle's counts and accuracies are float32 values)


# ------------------------------------------------------------------------------------------------------ oracle agreement
def test_set_losses_reproduce_the_oracle_and_ref_losses():
    for name in ("3x10x10", "4x3x64"):  # (the second: targets left unmatched)
        c = LC.SET[name]()
        N, Q = c["logits"][0].shape[:2]
        off = c["tgt_off"].tolist()
        xx = c["tgt_xx"].double()
        cxw = mo.span_xx_to_cxw(xx)
        xx = mo.span_cxw_to_xx(cxw)  # (the oracle derives the windows from the spans: criterion.py:95)
        mq = cpu_match(c, 0)
        targets = dict(norm_moment=[dict(moments=xx[off[b]:off[b + 1]]) for b in range(N)],
                       norm_span=[dict(spans=cxw[off[b]:off[b + 1]]) for b in range(N)])
        idx = []
        for b in range(N):
            t = torch.nonzero(mq[off[b]:off[b + 1]] >= 0).squeeze(1)
            idx.append((mq[off[b]:off[b + 1]][t].long(), t))
        cfg = dict(dataset_name="qvhighlights", eos_coef=0.1)
        lg, sp = c["logits"][0].double().requires_grad_(), c["spans"][0].double().requires_grad_()
        ours = LR.set_losses(lg, sp, cxw, xx, c["tgt_off"], mq, 0.1)
        with oracle_in_float64():
            lab = mo.loss_labels(lg, targets, idx, cfg)
        assert allclose(ours[2], lab["loss_label"])
        # (class_error is a float32 value by the oracle's own .float() on the hits: criterion.py:133)
        assert torch.allclose(ours[3], lab["class_error"].double(), rtol=1e-6, atol=0)
        assert allclose(*[torch.autograd.grad(v, lg)[0] for v in (ours[2], lab["loss_label"])])
        spn = mo.loss_spans(sp, targets, idx, cfg)  # (its gIoU is evaluated in float32: see the module docstring)
        assert allclose(ours[0], spn["loss_span"])
        assert allclose(*[torch.autograd.grad(v, sp, retain_graph=True)[0] for v in (ours[0], spn["loss_span"])])
        assert torch.allclose(ours[1], spn["loss_giou"].double(), rtol=1e-5, atol=1e-6)
        flat, keep = LR.matched(c["tgt_off"], mq, Q)
        src = LR.span_cxw_to_xx(sp.detach().reshape(-1, 2)[flat])
        iou, union = mo.temporal_iou(src, xx[keep])
        enc = (torch.max(src[:, None, 1], xx[keep][:, 1]) - torch.min(src[:, None, 0], xx[keep][:, 0])).clamp(min=0)
        assert allclose(LR.paired_giou(src, xx[keep]), torch.diag(iou - (enc - union) / enc))
        assert torch.allclose(LR.paired_giou(src, xx[keep]), torch.diag(mo.generalized_temporal_iou(src, xx[keep])).double(),
                              rtol=1e-5, atol=1e-6)
        # tests/ref_losses.py in float64
        sizes = torch.tensor(off[1:]) - torch.tensor(off[:-1])
        pair_of_t = torch.repeat_interleave(torch.arange(N), sizes)
        lg2, sp2 = lg.detach().clone().requires_grad_(), sp.detach().clone().requires_grad_()
        with oracle_in_float64():  # (its class weights are a tensor of the default dtype)
            theirs = R.set_losses(lg2, sp2, cxw, xx, pair_of_t, mq, 0.1)
        for a, b in zip(ours[:3], theirs[:3]):
            assert allclose(a, b)
        assert torch.allclose(ours[3], theirs[3].double(), rtol=1e-6, atol=0)
        w = (0.7, -1.3, 2.1)
        ours = LR.set_losses(lg, sp, cxw, xx, c["tgt_off"], mq, 0.1)
        ga = torch.autograd.grad(sum(wi * v for wi, v in zip(w, ours[:3])), (lg, sp))
        gb = torch.autograd.grad(sum(wi * v for wi, v in zip(w, theirs[:3])), (lg2, sp2))
        assert allclose(ga[0], gb[0]) and allclose(ga[1], gb[1])


@pytest.mark.parametrize("name", ["5x64_label12_P2", "4x128_P64_allpad_stage3", "17x75_noP"])
def test_saliency_reproduces_the_oracle(name):
    c = LC.SAL[name]()
    sp, sn = c["s_pos"].double().requires_grad_(), c["s_neg"].double().requires_grad_()
    ours = LR.saliency(sp, sn, c["label"], c["vmask"], c["pos_idx"], c["neg_idx"], c["rank_coef"], c["margin"])
    out = dict(saliency_scores=sp, neg_saliency_scores=sn)
    targets = dict(video_mask=c["vmask"], saliency_label=c["label"], pos_idx=c["pos_idx"], neg_idx=c["neg_idx"])
    cfg = dict(rank_coef=c["rank_coef"], use_triplet=c["pos_idx"] is not None, saliency_margin=c["margin"])
    with oracle_in_float64():
        theirs = mo.loss_saliency(out, targets, cfg)["loss_saliency"]
    assert allclose(ours, theirs)
    for a, b in zip(torch.autograd.grad(ours, (sp, sn)), torch.autograd.grad(theirs, (sp, sn))):
        assert allclose(a, b)


@pytest.mark.parametrize("name", ["5x20x9x30_tau0.07", "5x20x9x33_tau0.5", "3x5x4x260_tau0.5"])
def test_rec_ss_reproduces_the_oracle_and_ref_losses(name):
    c = LC.SS[name]()
    N = c["pv"].shape[0]
    g = torch.Generator().manual_seed(1)
    st = torch.rand(N, generator=g, dtype=F64) * 0.5
    mom = torch.stack([st, st + 0.1 + torch.rand(N, generator=g, dtype=F64) * 0.4], 1)
    pos = mo.generalized_temporal_iou(mom, mom) >= 0.3
    pv, ew = c["pv"].double().requires_grad_(), c["ew"].double().requires_grad_()
    ours = LR.rec_ss(pv, c["cmask"], ew, c["wmask"], pos, c["tau"])
    out = dict(projed_video_feat=pv, expanded_words_feat=ew, expanded_words_mask=c["wmask"])
    targets = dict(num_clips=torch.tensor([N]), norm_moment=mom, clip_mask=c["cmask"])
    with oracle_in_float64():
        theirs = mo.loss_rec_ss(out, targets, dict(dataset_name="charades", iou_gamma=0.3, recss_tau=c["tau"]))["loss_rec_ss"]
    mine = R.rec_ss(pv, c["cmask"], ew, c["wmask"], pos.double(), c["tau"])
    assert allclose(ours["loss"], theirs) and allclose(ours["loss"], mine)
    ga = torch.autograd.grad(ours["loss"], (pv, ew))
    for other in (theirs, mine):
        gb = torch.autograd.grad(other, (pv, ew))
        assert allclose(ga[0], gb[0]) and allclose(ga[1], gb[1])
    assert allclose(ours["rows"].mean(), ours["loss"])
    assert allclose(ours["sim"], torch.nn.functional.normalize(ours["cn"], dim=-1) @ ours["wn"].t() / c["tau"])


@pytest.mark.parametrize("name", ["C53", "C2049", "tie_C53", "nomask_C2048"])
def test_nll_and_its_reductions_reproduce_the_oracle_and_ref_losses(name):
    c = LC.NLL[name]()
    N, Lw = c["N"], c["Lw"]
    C = c["logit"].shape[1]
    mask = LR._nll_mask(c)
    logit = c["logit"].double().view(N, Lw, C).requires_grad_()
    label = c["label"].view(N, Lw)
    row_loss, lse, correct = LR.nll_smooth(logit.view(-1, C), c["label"], mask.reshape(-1))
    loss, acc = LR.rec_fw_reduce(row_loss.view(N, Lw), correct.view(N, Lw), mask)
    with oracle_in_float64():
        o = mo.loss_rec_fw(dict(recfw_words_logit=logit, words_mask=mask), dict(words_label=label), {})
    r = R.rec_fw(logit, label, mask.double())
    assert allclose(loss, o["loss_rec_fw"]) and allclose(loss, r[0])
    assert allclose(lse, torch.log(torch.exp(logit.view(-1, C)).sum(1)))
    if "tie" not in name:  # (which of two equal maxima argmax() returns is the build's choice; first_max states the first)
        assert allclose(acc, o["rec_fw_acc"]) and allclose(acc, r[1])
    else:
        assert correct.view(-1)[mask.reshape(-1)].tolist() == [i % 2 == 0 for i in range(N * Lw) if mask.reshape(-1)[i]]
    ga = torch.autograd.grad(0.7 * loss, logit, retain_graph=True)[0]
    assert allclose(ga, torch.autograd.grad(0.7 * o["loss_rec_fw"], logit)[0])
    assert allclose(ga, torch.autograd.grad(0.7 * r[0], logit)[0])
    rg = LR.rec_fw_rowgrad(mask, 0.7)  # the closed forms the kernels are compared with
    assert allclose(ga.view(-1, C), LR.nll_grad(logit.detach().view(-1, C), c["label"], lse.detach(), rg.reshape(-1)))
    assert allclose(rg, torch.autograd.grad(0.7 * loss, row_loss)[0].view(N, Lw) * mask)


@pytest.mark.parametrize("normalize", [True, False])
def test_text_prep_rowdot_and_weighted_sum_reproduce_their_formulas(normalize):
    c = LC.TEXT["5x9x300"]()
    w, m, s = LR.text_prep(c["x"], normalize)
    rw, rm, rs = R.post_process_text(c["x"].double(), normalize)
    assert allclose(w, rw) and torch.equal(m, rm) and allclose(s, rs)
    assert not m[4, 5] and w[4, 5].abs().sum() > 0   # the cancelling word: masked out, features kept
    assert m[4, 3] and (not normalize or abs(float(w[4, 3].norm()) - 1) > 0.5)   # under the clamp: not a unit vector
    d = LC.ROWDOT["2x9x300"]()
    assert allclose(LR.rowdot(d["a"], d["b"], d["scale"]), torch.einsum("nld,nd->nl", d["a"].double(), d["b"].double()) * d["scale"])
    v = LC.WSUM["n13"]()
    keep = [k for k in range(13) if k not in (3, 7)]
    assert allclose(LR.weighted_sum(v["vals"], v["weights"]), sum(v["vals"][k].double() * v["weights"][k].double() for k in keep))


# ------------------------------------------------------------------------------------------------------------ n_valid
def test_n_valid_is_the_function_on_the_first_pairs():
    c = LC.SAL["17x75_margin_exact"]()
    args = [c[n] for n in LR._SAL_KEYS]
    for k in (5, 17):
        a = LR.saliency(*args, c["rank_coef"], c["margin"], n_valid=k)
        assert torch.equal(a, LR.saliency(*LR.lead(k, *args), c["rank_coef"], c["margin"]))
    assert (LR.out_sal(c, 5)["ds_pos"][5:] == 0).all() and (LR.out_sal(c, 5)["ds_neg"][5:] == 0).all()
    c = LC.SS["5x20x9x30_tau0.07"]()
    a, b = LR.out_ss(c, 3), LR.out_ss(dict(c, pv=c["pv"][:3], cmask=c["cmask"][:3], ew=c["ew"][:3], wmask=c["wmask"][:3],
                                           pos=c["pos"][:3, :3]))
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["sim"], b["sim"]) and torch.equal(a["dpv"][:3], b["dpv"])
    assert (a["dpv"][3:] == 0).all() and (a["dew"][3:] == 0).all() and a["cn"].shape[0] == 5
    assert torch.equal(LR.out_ss(c, 5)["dew"], LR.out_ss(c)["dew"])
    c = LC.SET["70x12x4"]()
    mq = cpu_match(c, 0)
    k = 35
    T = int(c["tgt_off"][k])
    a = LR.out_set(c, 0, mq, k)
    cut = dict(c, logits=[c["logits"][0][:k]], spans=[c["spans"][0][:k]], tgt_off=c["tgt_off"][:k + 1], tgt_cxw=c["tgt_cxw"][:T],
               tgt_xx=c["tgt_xx"][:T])
    b = LR.out_set(cut, 0, mq[:T])
    assert torch.equal(a["out4"], b["out4"]) and torch.equal(a["dspans"][:k], b["dspans"]) and (a["dlogits"][k:] == 0).all()
    assert torch.equal(LR.out_set(c, 0, mq, 70)["dlogits"], LR.out_set(c, 0, mq)["dlogits"])
    c = LC.FW["33x7"]()
    a = LR.out_fw(c, 16)
    assert torch.equal(a["fw_loss"], LR.rec_fw_reduce(c["row_loss"][:16], c["correct"][:16], c["mask"][:16])[0])
    assert (a["rowgrad"][16:] == 0).all() and torch.equal(LR.out_fw(c, 33)["rowgrad"], LR.out_fw(c)["rowgrad"])


# ------------------------------------------------------------------------- the cases: inside the bounds, bounds <= 1e-4
OLD = 1e-4
ZERO = 1e-12  # an output (or a pair's gradient) that the reference leaves zero up to its own float64 rounding: no magnitude to
              # take 1e-4 of; the kernel is still held to the bound, which is built from the terms that cancel
# rec_ss of ONE pair can only be log(1 + 1e-6) ~ 1e-6: the float32 sum 1 + 1e-6 alone is 5 % off in it, so no float32
# evaluation is within 1e-4 of it, and N == 1 cannot be re-chosen.  Its value is held absolutely, the bound under 1e-6.
FORCED_TINY = {("1x1x1x4_tau0.5", "loss"): 1e-6, ("1x1x1x4_tau0.5", "rows"): 1e-6}


def runs(block):
    """(case name, n_valid) of a block: None, N (through the nv entries: the same statement) and every listed count"""
    for name, make in getattr(LC, block).items():
        c = make()
        for nv in [None] + c.get("nv", []):
            yield name, c, nv


def conditions(name, ref, bnd, alts, keys=None):
    bad = []
    for k in keys or ref:
        b, r = bnd[k].double(), ref[k].double().abs()
        if k in ("dpv", "dew"):
            # a pair whose mean is exactly 0 (the clamp branch) has a gradient 1e12 times the others': it is held to its own
            # largest magnitude and kept out of the others' scale, which is today's whole-tensor 2e-4 (test_criterion_gpu.py)
            b, r, old = b.expand_as(r).flatten(1).amax(1), r.flatten(1).amax(1), 2e-4
            clamp = (ref["cn" if k == "dpv" else "wn"][:r.shape[0]] == 0).all(1)
            r = torch.where(clamp, r, r[~clamp].max() if bool((~clamp).any()) else r)
        else:
            b, r, old = b.max().reshape(1), r.max().reshape(1), OLD
        case = name[0] if isinstance(name, tuple) else name
        allowed = torch.clamp(old * r, min=FORCED_TINY.get((case, k), 0.0))
        loose = (r > ZERO) & (b > allowed)
        if bool(loose.any()):
            i = int(torch.nonzero(loose)[0])
            bad.append((name, k, "bound %.3g > %g x %.3g" % (float(b[i]), old, float(r[i]))))
        for alt in alts:
            if k in alt and LR.excess(alt[k], ref[k], bnd[k]) > 1:
                bad.append((name, k, "float32 reference at %.3g bounds" % LR.excess(alt[k], ref[k], bnd[k])))
    return bad


def ref_losses_rec_fw_f32(c, nv, ties):
    """tests/ref_losses.py's rec_fw in float32 on the first k pairs: loss, accuracy and d (G_FW loss) / d logit by autograd"""
    N, Lw, C = c["N"], c["Lw"], c["logit"].shape[1]
    k = N if nv is None else nv
    logit = c["logit"].view(N, Lw, C)[:k].clone().requires_grad_()
    loss, acc = R.rec_fw(logit, c["label"].view(N, Lw)[:k], LR._nll_mask(c)[:k].float(), c["eps"])
    out = dict(fw_loss=loss.detach(), dlogit=LR._pad0(torch.autograd.grad(LR.G_FW * loss, logit)[0], N).view(N * Lw, C))
    if not ties:  # (which of two equal maxima max() returns is the build's choice)
        out["fw_acc"] = acc
    return out


def test_cases_nll():
    bad = []
    for name, c, nv in runs("NLL"):
        alts = [LR.out_nll(c, nv, F32), ref_losses_rec_fw_f32(c, nv, "tie" in name)]
        bad += conditions((name, nv), LR.out_nll(c, nv), LR.bnd_nll(c, nv), alts)
    assert not bad, bad


def test_cases_saliency():
    bad = []
    for name, c, nv in runs("SAL"):
        bad += conditions((name, nv), LR.out_sal(c, nv), LR.bnd_sal(c, nv), [LR.out_sal(c, nv, F32)])
    assert not bad, bad


def ref_losses_set_f32(c, layer, mq, k):
    off = c["tgt_off"].tolist()
    sizes = torch.tensor(off[1:k + 1]) - torch.tensor(off[:k])
    pair_of_t = torch.repeat_interleave(torch.arange(k), sizes)
    lg, sp = c["logits"][layer][:k].clone().requires_grad_(), c["spans"][layer][:k].clone().requires_grad_()
    T = off[k]
    ls = R.set_losses(lg, sp, c["tgt_cxw"][:T], c["tgt_xx"][:T], pair_of_t, mq[:T], c["eos_coef"])
    dl, ds = torch.autograd.grad(LR.G_SET[0] * ls[0] + LR.G_SET[1] * ls[1] + LR.G_SET[2] * ls[2], (lg, sp))
    N = c["logits"][layer].shape[0]
    return dict(out4=torch.stack([x.detach() for x in ls]), dlogits=LR._pad0(dl, N), dspans=LR._pad0(ds, N))


def test_cases_set_losses():
    bad = []
    for name, c, nv in runs("SET"):
        for layer in range(len(c["logits"])):
            mq = cpu_match(c, layer)
            k = c["logits"][layer].shape[0] if nv is None else nv
            alts = [LR.out_set(c, layer, mq, nv, F32), ref_losses_set_f32(c, layer, mq, k)]
            bad += conditions((name, layer, nv), LR.out_set(c, layer, mq, nv), LR.bnd_set(c, layer, mq, nv), alts)
    assert not bad, bad


def test_cases_rec_ss():
    bad = []
    for name, c, nv in runs("SS"):
        alts = [LR.out_ss(c, nv, F32)]
        k = c["pv"].shape[0] if nv is None else nv
        pv, ew = c["pv"][:k].clone().requires_grad_(), c["ew"][:k].clone().requires_grad_()
        loss = R.rec_ss(pv, c["cmask"][:k], ew, c["wmask"][:k], c["pos"][:k, :k].float(), c["tau"])
        dpv, dew = torch.autograd.grad(loss, (pv, ew))
        N = c["pv"].shape[0]
        alts.append(dict(loss=loss.detach(), dpv=LR.G_SS * LR._pad0(dpv, N), dew=LR.G_SS * LR._pad0(dew, N)))
        ref = LR.out_ss(c, nv)
        bad += conditions((name, nv), ref, LR.bnd_ss(c, nv), alts, [k for k in ref if k not in c.get("skip", ())])
    assert not bad, bad


def test_cases_rec_fw_rowdot_text_prep_weighted_sum():
    bad = []
    for name, c, nv in runs("FW"):  # (ref_losses.rec_fw starts from logits: it is the NLL cases' second evaluation)
        bad += conditions((name, nv), LR.out_fw(c, nv), LR.bnd_fw(c, nv), [LR.out_fw(c, nv, F32)])
    for name, make in LC.ROWDOT.items():
        c = make()
        a, b = c["a"].double().requires_grad_(), c["b"].double().requires_grad_()
        s = LR.rowdot(a, b, c["scale"])
        da, db = torch.autograd.grad((s * c["ds"].double()).sum(), (a, b))
        a32, b32 = c["a"].clone().requires_grad_(), c["b"].clone().requires_grad_()
        s32 = LR.rowdot(a32, b32, c["scale"], F32)
        da32, db32 = torch.autograd.grad((s32 * c["ds"]).sum(), (a32, b32))
        bad += conditions(name, dict(s=s.detach(), da=da, db=db), LR.rowdot_bounds(c["a"], c["b"], c["scale"], c["ds"]),
                          [dict(s=s32.detach(), da=da32, db=db32)])
    for name, make in LC.TEXT.items():
        for normalize in (True, False):
            c = make()
            w, m, s = LR.text_prep(c["x"], normalize)
            alts = []
            for fn in (lambda x, n: LR.text_prep(x, n, F32), R.post_process_text):
                w32, m32, s32 = fn(c["x"], normalize)
                assert torch.equal(m, m32), name
                alts.append(dict(words=w32, sent=s32))
            bad += conditions((name, normalize), dict(words=w, sent=s), LR.text_prep_bounds(c["x"], normalize), alts)
    for name, make in LC.WSUM.items():
        c = make()
        bad += conditions(name, dict(t=LR.weighted_sum(c["vals"], c["weights"])), dict(t=LR.weighted_sum_bounds(c["vals"], c["weights"])),
                          [dict(t=LR.weighted_sum(c["vals"], c["weights"], F32))])
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------- seeded defects
def old_metric(got, ref, tol=OLD):
    scale = max(float(ref.double().abs().max()), 1e-6)
    return float((got.double() - ref.double()).abs().max()) / scale < tol


DEFECT_BLOCK = {
    "nll_no_eps_over_C": "NLL", "recfw_capacity_N": "FW",
    "sal_no_argmax": "SAL", "sal_capacity_N": "SAL",
    "ss_no_1e-6": "SS", "ss_no_argmax": "SS", "ss_capacity_N": "SS", "ss_padding_column": "SS",
    "giou_inter_strict": "SET", "giou_enc_strict": "SET", "giou_onesided_tie": "SET", "set_eos_on_matched": "SET",
    "set_sum_T": "SET", "set_capacity_N": "SET",
}
# the run on which the bounds catch the defect and the older metric lets it through
SLIP_THROUGH = {"nll_no_eps_over_C": ("C5003", None), "ss_no_1e-6": ("4x1030x3x8_tau0.07", 2),
                "ss_no_argmax": ("4x1030x3x8_tau0.07", 2), "sal_no_argmax": ("2x1_far_near", None)}
# `>` for `>=` at a gIoU clamp changes nothing a test could see: raw_i == 0 means touching spans, whose union equals the
# enclosing span, so d inter cancels between -inter / union and -union / enc (d loss = d inter (1 / enc - 1 / union) = 0);
# raw_e == 0 needs both widths zero, where the reference is NaN (excluded).  Asserted below as bit-equality on every case.
BENIGN = {"giou_inter_strict", "giou_enc_strict"}

def block_eval(block, c, nv, dt):
    if block == "SET":
        out = {}
        for layer in range(len(c["logits"])):
            mq = cpu_match(c, layer)
            for k, v in LR.out_set(c, layer, mq, nv, dt).items():
                out["%s.%d" % (k, layer)] = v
        return out
    return dict(NLL=LR.out_nll, FW=LR.out_fw, SAL=LR.out_sal, SS=LR.out_ss)[block](c, nv, dt)


def block_bounds(block, c, nv):
    if block == "SET":
        out = {}
        for layer in range(len(c["logits"])):
            mq = cpu_match(c, layer)
            for k, v in LR.bnd_set(c, layer, mq, nv).items():
                out["%s.%d" % (k, layer)] = v
        return out
    return dict(NLL=LR.bnd_nll, FW=LR.bnd_fw, SAL=LR.bnd_sal, SS=LR.bnd_ss)[block](c, nv)


@pytest.mark.parametrize("defect", sorted(DEFECT_BLOCK))
def test_seeded_defects(defect):
    """a float32 copy of the reference with one defect falls outside the derived bounds on at least one listed case (but for
    BENIGN, which says why); on the runs of SLIP_THROUGH the older whole-tensor metric lets it through"""
    block = DEFECT_BLOCK[defect]
    worst, caught, old_caught = 0.0, set(), set()
    assert not LR.DEFECTS
    for name, c, nv in runs(block):
        ref, bnd = block_eval(block, c, nv, F64), block_bounds(block, c, nv)
        LR.DEFECTS.add(defect)
        try:
            got = block_eval(block, c, nv, F32)
        finally:
            LR.DEFECTS.clear()
        if defect in BENIGN:
            clean = block_eval(block, c, nv, F32)
            assert all(torch.equal(got[k], clean[k]) for k in ref), (name, nv)
            continue
        for k in ref:
            x = LR.excess(got[k], ref[k], bnd[k])
            worst = max(worst, x)
            if x > 1:
                caught.add((name, nv))
            if not old_metric(got[k], ref[k], 2e-4 if k in ("dpv", "dew") else OLD):
                old_caught.add((name, nv))
    if defect in BENIGN:
        return
    assert caught, (defect, worst)
    if defect in SLIP_THROUGH:
        assert SLIP_THROUGH[defect] in caught and SLIP_THROUGH[defect] not in old_caught


# ------------------------------------------------------------------------------------------------------ the tie batch
def test_tie_batch_has_the_same_finite_gradients_in_float32_and_float64():
    c = LC.SET["ties"]()
    grads = {}
    for dt in (F32, F64):
        sp = c["spans"][0].to(dt).reshape(7, 2).requires_grad_()
        giou = LR.paired_giou(LR.span_cxw_to_xx(sp), c["tgt_xx"].to(dt))
        l1 = (sp - c["tgt_cxw"].to(dt)).abs().sum()
        grads[dt] = torch.autograd.grad((1 - giou).sum() + l1, sp)[0]
        assert torch.isfinite(grads[dt]).all()
    assert torch.equal(grads[F32].double(), grads[F64])
    g = grads[F64]
    assert (g[4] == 0).all()  # identical spans: every tie splits evenly and cancels, the L1 sign is 0 at 0
    # right ends equal (pair 0): d/dx2 of min(x2, g2) and of max(x2, g2) are 1/2 each -- not the one-sided 1 or 0
    x = torch.tensor([0.75], dtype=F64, requires_grad=True)
    y = torch.tensor([0.75], dtype=F64)
    assert torch.autograd.grad(torch.min(x, y).sum(), x)[0].item() == 0.5
    assert torch.autograd.grad(torch.max(x, y).sum(), x)[0].item() == 0.5
    z = torch.zeros(1, dtype=F64, requires_grad=True)
    assert torch.autograd.grad(z.clamp(min=0).sum(), z)[0].item() == 1.0   # touching spans: raw_i == 0 passes the gradient
    assert torch.autograd.grad(z.abs().sum(), z)[0].item() == 0.0
    LR.DEFECTS.add("giou_onesided_tie")
    try:
        sp = c["spans"][0].double().reshape(7, 2).requires_grad_()
        one = torch.autograd.grad((1 - LR.paired_giou(LR.span_cxw_to_xx(sp), c["tgt_xx"].double())).sum(), sp)[0]
    finally:
        LR.DEFECTS.clear()
    sp = c["spans"][0].double().reshape(7, 2).requires_grad_()
    even = torch.autograd.grad((1 - LR.paired_giou(LR.span_cxw_to_xx(sp), c["tgt_xx"].double())).sum(), sp)[0]
    assert not torch.equal(one[0], even[0]) and not torch.equal(one[1], even[1]) and torch.equal(one[3], even[3])
