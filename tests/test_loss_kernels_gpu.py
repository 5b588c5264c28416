"""Every loss entry of csrc/criterion.hip, csrc/losses.hip and csrc/loss_bodies.hpp against the fp64 reference of
tests/loss_ref.py on the MI355X, forward and backward, in its three forms -- the separate entry, the `_nv` entry with a device
count (n_valid == N and 0 < n_valid < N) and the merged kernels.criterion_fwd / criterion_bwd (with and without a count) --
on the named cases of tests/loss_cases.py.  Each output is held to the bound that loss_ref derives for it from the inputs
(per element or row, never from a kernel's output); where a kernel must write an exact zero -- masked rows of dlogit, padded
clips of ds_pos / ds_neg, masked clips and words of dpv / dew, unmatched queries, every gradient row of a padding pair -- the
bound is 0 and the check is equality.  The reference is evaluated on the CPU (tests/test_loss_ref_cpu.py pins it there).

ops.rowdot cannot reach the backward kernel at D % 4 != 0 (its forward refuses first), so D = 6 goes to kernels.rowdot_bwd
directly.  HEADROOM keeps each check's largest error in units of its bound; tools/loss_headroom.py prints it as the table of
profiles/loss_kernels/README.md."""
import pytest
import torch

import loss_cases as LC
import loss_ref as LR

pytestmark = pytest.mark.gpu
COSTS = (10.0, 1.0, 4.0)
HEADROOM = []  # (kernels, case, form, output, largest bound, largest error / bound)


def dev():
    return torch.device("cuda:0")


def to_dev(c):
    out = {}
    for k, v in c.items():
        if torch.is_tensor(v):
            out[k] = v.to(dev()).contiguous()
        elif isinstance(v, list) and v and torch.is_tensor(v[0]):
            out[k] = [t.to(dev()).contiguous() for t in v]
        else:
            out[k] = v
    return out


def count(k):
    return None if k is None else torch.tensor([k], dtype=torch.int32, device=dev())


def f32(*vals):
    return torch.tensor(list(vals), dtype=torch.float32, device=dev())


def forms(c, N):
    """(label, n_valid of the reference, n_valid handed to the kernel): no count, the count N, every listed 0 < k < N"""
    return [("none", None, None), ("nv=N", None, N)] + [("nv=%d" % k, k, k) for k in c.get("nv", [])]


def hold(kernel, case, form, got, ref, bnd):
    """every output of `ref` within its bound; the keys of `got` may be a subset"""
    bad = []
    for k, v in got.items():
        x = LR.excess(v.detach().cpu(), ref[k], bnd[k])
        HEADROOM.append((kernel, case, form, k, float(bnd[k].max()), x))
        if not x <= 1:
            bad.append((k, x))
    assert not bad, (kernel, case, form, bad)


def held_total(total, lv, w):
    """the weighted total of the merged forward against the fp64 sum of its own slots"""
    ref = LR.weighted_sum(lv.cpu(), w.cpu())
    assert LR.excess(total.cpu(), ref, LR.weighted_sum_bounds(lv.cpu(), w.cpu())) <= 1


# ------------------------------------------------------------------------------------------------------------------ NLL
@pytest.mark.parametrize("name", sorted(LC.NLL))
def test_nll(name):
    from mesm_amd import kernels as kn
    c = LC.NLL[name]()
    d = to_dev(c)
    N, Lw, C = c["N"], c["Lw"], c["logit"].shape[1]
    mask2 = LR._nll_mask(d)
    for label, k, kd in forms(c, N):
        ref, bnd = LR.out_nll(c, k), LR.bnd_nll(c, k)
        row_loss, row_lse, correct = kn.nll_smooth_fwd(d["logit"], d["label"], d["mask"], c["eps"])
        out2 = torch.zeros(2, device=dev())
        kn.rec_fw_reduce(row_loss, correct, mask2, out2, n_valid=count(kd))
        rg = kn.rec_fw_rowgrad(mask2, f32(LR.G_FW), n_valid=count(kd))
        dl = kn.nll_smooth_bwd(d["logit"], d["label"], row_lse, rg, c["eps"])
        hold("nll_smooth / rec_fw", name, label, dict(row_loss=row_loss, lse=row_lse, correct=correct, fw_loss=out2[0], fw_acc=out2[1],
                                                      rowgrad=rg, dlogit=dl), ref, bnd)
        # the merged launches: slot 0 the loss (weight G_FW), slot 1 the accuracy (logged: weight 0)
        lv, w = torch.full((3,), 7.0, device=dev()), f32(LR.G_FW, 0.0, 0.0)
        fw = dict(logit=d["logit"].view(N, Lw, C), label=d["label"], mask=mask2, eps=c["eps"], slot=0)
        total, saved = kn.criterion_fwd(lv, w, N, n_valid=count(kd), recfw=fw)
        dl2 = torch.full_like(d["logit"], 7.0)
        kn.criterion_bwd(f32(1.0), w, N, n_valid=count(kd),
                         recfw=dict(fw, row_lse=saved["row_lse"], dlogit=dl2.view(N, Lw, C)))
        hold("criterion_fwd/bwd: rec_fw", name, label, dict(row_loss=saved["_staging"][0], lse=saved["row_lse"], correct=saved["_staging"][1],
                                                            fw_loss=lv[0], fw_acc=lv[1], dlogit=dl2), ref, bnd)
        assert lv[2] == 7.0
        held_total(total, lv, w)


# ------------------------------------------------------------------------------------------------------------- saliency
SAL_ARGS = ("s_pos", "s_neg", "label", "vmask", "pos_idx", "neg_idx", "rank_coef", "margin")


@pytest.mark.parametrize("name", sorted(LC.SAL))
def test_saliency(name):
    from mesm_amd import kernels as kn
    c = LC.SAL[name]()
    d = to_dev(c)
    N = c["s_pos"].shape[0]
    args = [d[k] for k in SAL_ARGS]
    for label, k, kd in forms(c, N):
        ref, bnd = LR.out_sal(c, k), LR.bnd_sal(c, k)
        out = kn.saliency_loss_fwd(*args, n_valid=count(kd))
        dp, dn = kn.saliency_loss_bwd(*args, f32(LR.G_SAL), n_valid=count(kd))
        hold("saliency_loss", name, label, dict(loss=out[0], ds_pos=dp, ds_neg=dn), ref, bnd)
        lv, w = torch.full((2,), 7.0, device=dev()), f32(LR.G_SAL, 0.0)
        sal = dict({k2: d[k2] for k2 in SAL_ARGS}, slot=0)
        total, _ = kn.criterion_fwd(lv, w, N, n_valid=count(kd), sal=sal)
        dp2, dn2 = torch.full_like(d["s_pos"], 7.0), torch.full_like(d["s_neg"], 7.0)
        kn.criterion_bwd(f32(1.0), w, N, n_valid=count(kd), sal=dict(sal, ds_pos=dp2, ds_neg=dn2))
        hold("criterion_fwd/bwd: saliency", name, label, dict(loss=lv[0], ds_pos=dp2, ds_neg=dn2), ref, bnd)
        assert lv[1] == 7.0
        held_total(total, lv, w)


def test_saliency_refuses_641_clips():
    from mesm_amd import _lib, kernels as kn
    N, L = 2, 641
    z = torch.zeros(N, L, device=dev())
    out = torch.full((1,), 7.0, device=dev())
    with pytest.raises(_lib.MesmError, match="mesm_saliency_loss_fwd"):
        kn.saliency_loss_fwd(z, z, z.double(), z.bool(), None, None, 12.0, 0.2, out=out)
    dp, dn = torch.full_like(z, 7.0), torch.full_like(z, 7.0)
    with pytest.raises(_lib.MesmError, match="mesm_saliency_loss_bwd"):
        kn.saliency_loss_bwd(z, z, z.double(), z.bool(), None, None, 12.0, 0.2, f32(1.0), out=(dp, dn))
    torch.cuda.synchronize()
    assert out.item() == 7.0 and bool((dp == 7.0).all()) and bool((dn == 7.0).all())  # nothing was launched


# ----------------------------------------------------------------------------------------------------------- set losses
@pytest.mark.parametrize("name", sorted(LC.SET))
def test_set_losses(name):
    from mesm_amd import kernels as kn
    c = LC.SET[name]()
    d = to_dev(c)
    nl = len(c["logits"])
    N, Q, _ = c["logits"][0].shape
    tg = (d["tgt_cxw"], d["tgt_xx"], d["tgt_off"])
    g3 = f32(*LR.G_SET)
    mq_ref = [kn.match(d["logits"][l], d["spans"][l], *tg, c["tmax"], *COSTS) for l in range(nl)]  # (pinned to scipy)
    for label, k, kd in forms(c, N):
        T = int(c["tgt_off"][N if k is None else k])
        outs = [torch.zeros(4, device=dev()) for _ in range(nl)]
        mqs = kn.set_loss_fwd_layers([(d["logits"][l], d["spans"][l], outs[l]) for l in range(nl)], *tg, c["tmax"], *COSTS,
                                     c["eos_coef"], n_valid=count(kd))
        lv, w = torch.full((4 * nl + 1,), 7.0, device=dev()), f32(*(list(LR.G_SET) + [0.0]) * nl, 0.0)
        sl = dict(Q=Q, Tmax=c["tmax"], w_span=COSTS[0], w_giou=COSTS[1], w_class=COSTS[2], eos_coef=c["eos_coef"], tgt_cxw=tg[0],
                  tgt_xx=tg[1], tgt_off=tg[2])
        total, saved = kn.criterion_fwd(lv, w, N, n_valid=count(kd), set_losses=dict(sl, layers=[(d["logits"][l], d["spans"][l], 4 * l)
                                                                                                  for l in range(nl)]))
        grads = [(torch.full_like(d["logits"][l], 7.0), torch.full_like(d["spans"][l], 7.0)) for l in range(nl)]
        kn.criterion_bwd(f32(1.0), w, N, n_valid=count(kd),
                         set_losses=dict(sl, layers=[(d["logits"][l], d["spans"][l], saved["match"][l]) + grads[l] + (4 * l,)
                                                     for l in range(nl)]))
        for l in range(nl):
            out4 = torch.zeros(4, device=dev())
            mq = kn.set_loss_fwd(d["logits"][l], d["spans"][l], *tg, c["tmax"], *COSTS, c["eos_coef"], out4, n_valid=count(kd))
            for m in (mq, mqs[l], saved["match"][l]):
                assert torch.equal(m[:T], mq_ref[l][:T]), (name, label, l)
            ref, bnd = LR.out_set(c, l, mq_ref[l].cpu(), k), LR.bnd_set(c, l, mq_ref[l].cpu(), k)
            dl, ds = kn.set_loss_bwd(d["logits"][l], d["spans"][l], *tg, mq, c["eos_coef"], g3, n_valid=count(kd))
            hold("set_loss_fwd / set_loss_bwd", name, label, dict(out4=out4, dlogits=dl, dspans=ds), ref, bnd)
            hold("set_loss_fwd_layers", name, label, dict(out4=outs[l]), ref, bnd)
            hold("criterion_fwd/bwd: set losses", name, label, dict(out4=lv[4 * l:4 * l + 4], dlogits=grads[l][0], dspans=grads[l][1]),
                 ref, bnd)
        assert lv[4 * nl] == 7.0
        held_total(total, lv, w)


# --------------------------------------------------------------------------------------------------------------- rec_ss
@pytest.mark.parametrize("name", sorted(LC.SS))
def test_rec_ss(name):
    from mesm_amd import kernels as kn
    c = LC.SS[name]()
    d = to_dev(c)
    N, Lv, D = c["pv"].shape
    Le = c["ew"].shape[1]
    pos8 = d["pos"].to(torch.uint8).contiguous()

    def outputs(saved, loss, dpv, dew, k):
        cn, wn, stats, sim = saved
        n = N if k is None else k
        o = dict(loss=loss, cn=cn, wn=wn, sim=sim[:n, :n], rows=stats.view(-1)[4 * N:4 * N + n], dpv=dpv, dew=dew)
        return {k2: v for k2, v in o.items() if k2 not in c.get("skip", ())}  # (a forward-only case: loss_cases.py says why)

    for label, k, kd in forms(c, N):
        ref, bnd = LR.out_ss(c, k), LR.bnd_ss(c, k)
        out = torch.zeros(1, device=dev())
        saved = kn.rec_ss_fwd(d["pv"], d["cmask"], d["ew"], d["wmask"], pos8, c["tau"], out, n_valid=count(kd))
        dpv, dew = kn.rec_ss_bwd(saved, pos8, d["cmask"], d["wmask"], Lv, Le, c["tau"], f32(LR.G_SS), n_valid=count(kd))
        hold("rec_ss_fwd / rec_ss_bwd", name, label, outputs(saved, out[0], dpv, dew, k), ref, bnd)
        lv, w = torch.full((2,), 7.0, device=dev()), f32(LR.G_SS, 0.0)
        ss = dict(cmask=d["cmask"], wmask=d["wmask"], pos=pos8, tau=c["tau"], slot=0)
        total, sv = kn.criterion_fwd(lv, w, N, n_valid=count(kd), recss=dict(ss, pv=d["pv"], ew=d["ew"]))
        dpv2, dew2 = torch.full_like(d["pv"], 7.0), torch.full_like(d["ew"], 7.0)
        kn.criterion_bwd(f32(1.0), w, N, n_valid=count(kd), recss=dict(ss, saved=sv["recss"], Lv=Lv, Le=Le, dpv=dpv2, dew=dew2))
        hold("criterion_fwd/bwd: rec_ss", name, label, outputs(sv["recss"], lv[0], dpv2, dew2, k), ref, bnd)
        assert lv[1] == 7.0
        held_total(total, lv, w)


def test_rec_ss_refusals():
    """D = 1025 (the 16-slice row of a lane holds 1024 columns) and a similarity block past the backward's LDS check"""
    from mesm_amd import _lib, kernels as kn
    N, L, D = 2, 3, 1025
    pv, m = torch.zeros(N, L, D, device=dev()), torch.ones(N, L, dtype=torch.bool, device=dev())
    pos = torch.eye(N, dtype=torch.uint8, device=dev())
    out = torch.full((1,), 7.0, device=dev())
    with pytest.raises(_lib.MesmError, match="mesm_rec_ss_fwd"):
        kn.rec_ss_fwd(pv, m, pv, m, pos, 0.5, out)
    N, D = 120, 8  # 5 N^2 bytes of LDS: 72,000 > 65,536
    saved = (torch.zeros(N, D, device=dev()), torch.zeros(N, D, device=dev()), torch.ones(2 * N, 4, device=dev()),
             torch.zeros(N, N, device=dev()))
    m = torch.ones(N, L, dtype=torch.bool, device=dev())
    with pytest.raises(_lib.MesmError, match="mesm_rec_ss_bwd"):
        kn.rec_ss_bwd(saved, torch.eye(N, dtype=torch.uint8, device=dev()), m, m, L, L, 0.5, f32(1.0))
    torch.cuda.synchronize()
    assert out.item() == 7.0


# --------------------------------------------------------------------------------------------------- rec_fw reductions
@pytest.mark.parametrize("name", sorted(LC.FW))
def test_rec_fw_reduce_and_rowgrad(name):
    from mesm_amd import kernels as kn
    c = LC.FW[name]()
    d = to_dev(c)
    N = c["mask"].shape[0]
    for label, k, kd in forms(c, N):
        out2 = torch.zeros(2, device=dev())
        kn.rec_fw_reduce(d["row_loss"].reshape(-1), d["correct"].to(torch.uint8).reshape(-1), d["mask"], out2, n_valid=count(kd))
        rg = kn.rec_fw_rowgrad(d["mask"], f32(LR.G_FW), n_valid=count(kd))
        hold("rec_fw_reduce / rec_fw_rowgrad", name, label, dict(fw_loss=out2[0], fw_acc=out2[1], rowgrad=rg.view(N, -1)),
             LR.out_fw(c, k), LR.bnd_fw(c, k))


# --------------------------------------------------------------------------------------------------------------- rowdot
@pytest.mark.parametrize("name", sorted(LC.ROWDOT))
def test_rowdot(name):
    from mesm_amd import ops
    c = LC.ROWDOT[name]()
    d = to_dev(c)
    a, b = d["a"].clone().requires_grad_(), d["b"].clone().requires_grad_()
    s = ops.rowdot(a, b, c["scale"])
    (s * d["ds"]).sum().backward()
    a64, b64 = c["a"].double().requires_grad_(), c["b"].double().requires_grad_()
    r = LR.rowdot(a64, b64, c["scale"])
    da, db = torch.autograd.grad((r * c["ds"].double()).sum(), (a64, b64))
    hold("rowdot_fwd / rowdot_bwd", name, "none", dict(s=s, da=a.grad, db=b.grad), dict(s=r.detach(), da=da, db=db),
         LR.rowdot_bounds(c["a"], c["b"], c["scale"], c["ds"]))


def test_rowdot_refuses_the_forward_at_D6_and_runs_the_backward():
    from mesm_amd import _lib, kernels as kn, ops
    g = torch.Generator().manual_seed(8)
    a, b, ds = torch.randn(3, 5, 6, generator=g), torch.randn(3, 6, generator=g), torch.randn(3, 5, generator=g)
    with pytest.raises(_lib.MesmError, match="mesm_rowdot_fwd"):
        ops.rowdot(a.to(dev()), b.to(dev()), 0.25)
    da, db = kn.rowdot_bwd(a.to(dev()), b.to(dev()), ds.to(dev()), 0.25)  # the scalar columns of the backward
    a64, b64 = a.double().requires_grad_(), b.double().requires_grad_()
    ra, rb = torch.autograd.grad((LR.rowdot(a64, b64, 0.25) * ds.double()).sum(), (a64, b64))
    hold("rowdot_bwd", "3x5x6", "none", dict(da=da, db=db), dict(da=ra, db=rb), LR.rowdot_bounds(a, b, 0.25, ds))


# ------------------------------------------------------------------------------------------------------------ text_prep
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("name", sorted(LC.TEXT))
def test_text_prep(name, normalize):
    from mesm_amd import kernels as kn
    c = LC.TEXT[name]()
    w, m, s = kn.text_prep(c["x"].to(dev()), normalize)
    rw, rm, rs = LR.text_prep(c["x"], normalize)
    assert torch.equal(m.cpu(), rm)
    hold("text_prep", name, "normalize=%s" % normalize, dict(words=w, sent=s), dict(words=rw, sent=rs),
         LR.text_prep_bounds(c["x"], normalize))
    if c["x"].shape[1] >= 9:  # the cancelling word: masked out, its features kept
        assert not m[-1, 5] and float(w[-1, 5].abs().sum()) > 0 and bool(m[-1, 3])


# --------------------------------------------------------------------------------------------------------- weighted sum
@pytest.mark.parametrize("name", sorted(LC.WSUM))
def test_weighted_sum_and_scale_vec(name):
    from mesm_amd import kernels as kn
    c = LC.WSUM[name]()
    v, w = c["vals"].to(dev()), c["weights"].to(dev())
    hold("weighted_sum", name, "none", dict(t=kn.weighted_sum(v, w)), dict(t=LR.weighted_sum(c["vals"], c["weights"])),
         dict(t=LR.weighted_sum_bounds(c["vals"], c["weights"])))
    ref = c["g"] * c["weights"].double()
    hold("scale_vec", name, "none", dict(gv=kn.scale_vec(f32(c["g"]), w)), dict(gv=ref), dict(gv=LR.U32 * ref.abs()))


def test_scale_vec_refuses_257_slots():
    from mesm_amd import _lib, kernels as kn
    with pytest.raises(_lib.MesmError, match="mesm_scale_vec"):
        kn.scale_vec(f32(1.0), torch.ones(257, device=dev()))
