"""Every mask option of the attention core (MesmAttnArgs) on every kernel family that accepts it, against the fp64
reference of tests/attn_ref.py: the T2V quirk with mask_group and mask_mod, split heads with k_add, the causal mask,
dropout, the lse output and rows whose keys are all masked.

Besides the normwise 1e-4 of tests/test_kernels_gpu.py, every row is held to its own first-order float32 bound
(attn_ref.py states the derivation), the backward runs into NaN-prefilled gradients (every element must be written),
the dk / dv rows of keys masked for every query of their (b, h) must be exactly 0, and each case runs a second time as
two problems of one launch phase (kn.phase(): the grouped entry points and their other workgroup shapes).

Families are reached by shape alone (attention.hip mesm_attn_fwd / mesm_attn_bwd, attention_blk.hip *_ok predicates,
attention_mfma.hip mesm_attn_mfma_ok / mesm_attn_mfma_bwd_ok); the comment beside each case names the forward / backward
family it takes.  The matrix-core FORWARD (attention_mfma.hip) is unreachable by shape while the 16 x 16-block forward is
on (its default): every dk = dv = 32 shape it accepts, the block forward or its long form takes first."""
import contextlib
import ctypes

import pytest
import torch

from attn_ref import attention, causal_mask, heads, interleave, kpad_mask, quirk_mask, row_bounds, row_err

pytestmark = pytest.mark.gpu

TOL = 1e-4


def dev():
    return torch.device("cuda:0")


def gen(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dev())


def make_pad(B, L, seed):
    """(B, L) bool on the CPU, True = padded; every row keeps position 0, row 0 is full"""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    return torch.arange(L)[None, :] >= lens[:, None]


def rel_err(a, b):
    a, b = a.double(), b.double()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-6)


class Problem:
    """One attention problem: fp32 inputs in the layout the kernels read, the packed fp32 view the reference reads
    (qf, kf, vf: [q || q2], [k + k_add || k2] for split heads) and the effective mask (B, H, Lq, Lk)."""

    def __init__(self, seed, B, H, Lq, Lk, dk, dv, masked, kpad=None, qpad=None, group=0, drop_p=0.0, causal=False,
                 split=None):
        self.B, self.H, self.Lq, self.Lk, self.dk, self.dv = B, H, Lq, Lk, dk, dv
        self.kpad = kpad.to(torch.uint8).to(dev()) if kpad is not None else None
        self.qpad = qpad.to(torch.uint8).to(dev()) if qpad is not None else None
        self.group, self.causal, self.split = group, causal, split
        self.masked = masked.to(dev())
        self.scale = dk ** -0.5
        self.do = gen((B, Lq, H * dv), seed + 9)
        self.q2 = self.k2 = self.k_add = None
        if split is None:
            self.q, self.k, self.v = gen((B, Lq, H * dk), seed), gen((B, Lk, H * dk), seed + 1), gen((B, Lk, H * dv), seed + 2)
            self.qf, self.kf, self.vf = self.q, self.k, self.v
        else:
            # the decoder's layout (ops.py cross-attention): one (B, Lk, 3d) buffer [k content | v | k pos] read in place
            # with row stride 3d; k_add = the k pos slice itself on layer 0 ("alias"), or another tensor ("own")
            d = H * dk // 2
            assert H * dv == d
            self.kvp = gen((B, Lk, 3 * d), seed + 1)
            self.q, self.q2 = gen((B, Lq, d), seed), gen((B, Lq, d), seed + 3)
            self.k, self.v, self.k2 = self.kvp[..., :d], self.kvp[..., d:2 * d], self.kvp[..., 2 * d:]
            if split == "alias":
                self.k_add = self.k2
            elif split == "own":
                self.k_add = gen((B, Lk, 3 * d), seed + 4)[..., 2 * d:]
            ksum = self.k + self.k_add if self.k_add is not None else self.k
            self.qf, self.kf, self.vf = interleave(self.q, self.q2, H), interleave(ksum, self.k2, H), self.v.contiguous()
        self.drop = (drop_p, 1000 + seed)
        self.mult = None
        if drop_p > 0:
            from mesm_amd import kernels as kn
            # the kernels' counter hash, index ((b*H + h)*Lq + i)*Lk + j with the GLOBAL b (stacked groups included)
            self.mult = kn.dropout(torch.ones(B * H * Lq * Lk, device=dev()), drop_p, self.drop[1]).view(B, H, Lq, Lk)

    def fwd(self):
        from mesm_amd import kernels as kn
        return kn.attn_fwd(self.q, self.k, self.v, self.H, kpad=self.kpad, qpad=self.qpad, scale=self.scale,
                           drop=self.drop, group=self.group, causal=self.causal, q2=self.q2, k2=self.k2,
                           k_add=self.k_add)

    def bwd_into(self, o, lse):
        """attn_bwd_into with every gradient prefilled with NaN (dq / dq2 with zeros where the shape ADDS into them)"""
        from mesm_amd import kernels as kn
        nan = float("nan")
        adds = kn.attn_bwd_adds_dq(self.B, self.H, self.Lq, self.Lk, self.dk, self.dv, split=self.split is not None)
        fill = 0.0 if adds else nan
        if self.split is None:
            g = [torch.full_like(self.q, fill), torch.full_like(self.k, nan), torch.full_like(self.v, nan)]
            kn.attn_bwd_into(self.do, self.q, self.k, self.v, o, lse, self.H, *g, kpad=self.kpad, qpad=self.qpad,
                             scale=self.scale, drop=self.drop, group=self.group)
            return g
        d = self.q.shape[2]
        dq2x = torch.full((2,) + tuple(self.q.shape), fill, device=dev())
        dkvp = torch.full_like(self.kvp, nan)
        g = [dq2x[0], dkvp[..., :d], dkvp[..., d:2 * d], dq2x[1], dkvp[..., 2 * d:]]
        kn.attn_bwd_into(self.do, self.q, self.k, self.v, o, lse, self.H, g[0], g[1], g[2], kpad=self.kpad,
                         scale=self.scale, drop=self.drop, q2=self.q2, k2=self.k2, dq2=g[3], dk2=g[4], k_add=self.k_add)
        return g

    def packed_grads(self, g):
        """-> dq, dk, dv of the packed (interleaved) view"""
        if self.split is None:
            return g
        return interleave(g[0], g[3], self.H), interleave(g[1], g[4], self.H), g[2]


def margin(tag, name, err, bound):
    """largest err / bound (printed: the PR reports them); asserts the bound.  A zero bound (a row whose unmasked
    keys were all dropped: o = 0) admits no error at all."""
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, float("inf"), 0.0))
    r = r.max().item() if err.numel() else 0.0
    print("MARGIN %s %s %.3g" % (tag, name, r))
    assert r <= 1.0, (tag, name, r)


def check_fwd(p, o, lse, tag):
    H = p.H
    full = p.masked.all(-1)  # (B, H, Lq): rows whose keys are all masked
    ref, ref_lse = attention(p.qf, p.kf, p.vf, H, p.masked, p.scale, p.mult)
    bd = row_bounds(p.qf, p.kf, p.vf, H, p.masked, p.scale, p.mult, p16=p.causal)
    # the header's promise: NaN in o, a non-finite lse -- and only there
    oh = heads(o, H)
    assert torch.equal(oh.isnan().any(-1), full) and bool(oh.isnan().all(-1)[full].all()), tag
    assert bool(torch.isfinite(oh).all(-1)[~full].all()), tag
    assert torch.equal(~torch.isfinite(lse), full), tag
    ok = ~full
    margin(tag, "o", row_err(o, ref, H)[ok], bd["o"][ok])
    margin(tag, "lse", (lse.double() - ref_lse)[ok].abs(), bd["lse"][ok])
    if not p.causal:  # (the causal forward's fp16 probabilities are held to their own bound above only)
        okr = ok.transpose(1, 2).repeat_interleave(p.dv, -1).reshape(o.shape)
        assert rel_err(o[okr], ref[okr]) < TOL, tag


def check_bwd(p, o, lse, g, tag):
    H = p.H
    assert not bool(p.masked.all(-1).any())
    for t in g:
        assert bool(torch.isfinite(t).all()), tag  # every element written (NaN sentinels), dummy rows finite
    dq, dk, dv = p.packed_grads(g)
    qd, kd, vd = (t.detach().double().requires_grad_(True) for t in (p.qf, p.kf, p.vf))
    ref, _ = attention(qd, kd, vd, H, p.masked, p.scale, p.mult)
    ref.backward(p.do.double())
    bd = row_bounds(p.qf, p.kf, p.vf, H, p.masked, p.scale, p.mult, do=p.do)
    # keys masked for EVERY query of their (b, h): P = 0 in the whole column, their gradient rows are exactly 0
    cols = p.masked.all(-2)  # (B, H, Lk)
    assert bool((heads(dk, H)[cols] == 0).all()) and bool((heads(dv, H)[cols] == 0).all()), tag
    for name, x, r in (("dq", dq, qd.grad), ("dk", dk, kd.grad), ("dv", dv, vd.grad)):
        margin(tag, name, row_err(x, r, H), bd[name])
        assert rel_err(x, r) < TOL, (tag, name)


def run(probs, grouped, backward=True, mod=None):
    """forward (and backward) of every problem, one plain launch each or all in one launch phase per direction"""
    from mesm_amd import kernels as kn
    ctx = kn.phase if grouped else contextlib.nullcontext
    mod_t = torch.tensor([mod], dtype=torch.int32, device=dev()) if mod is not None else None
    kn.set_mask_mod(mod_t)
    try:
        with ctx():
            fw = [p.fwd() for p in probs]
        gs = None
        if backward:
            with ctx():
                gs = [p.bwd_into(o, lse) for p, (o, lse) in zip(probs, fw)]
        torch.cuda.synchronize()
    finally:
        kn.set_mask_mod(None)
    return fw, gs


def copies(grouped, make):
    """the problem alone, or two problems with other data sharing the launches of one phase"""
    return [make(0), make(100)] if grouped else [make(0)]


# ------------------------------------------------------------------------------------------- T2V quirk: group, modulus
QUIRK_CASES = [
    # B, H, Lq, Lk, dk, dv, G, n (modulus, < G)             forward family / backward family
    (64, 8, 75, 32, 32, 32, 32, 7),    # C3a enhance, positive + negative pass: blk short (dk 32, Lk <= 128) / blk short
    (128, 8, 75, 33, 32, 32, 64, 40),  # stacked 64-row passes, ragged key block: blk short / blk short
    (8, 8, 300, 40, 32, 32, 4, 3),     # blk short / matrix-core long-Lq (Lq >= 256, Lk <= 128)
    (4, 8, 513, 16, 32, 32, 2, 1),     # C5 513 x 16: blk short / matrix-core long-Lq
    (4, 4, 513, 513, 32, 32, 2, 1),    # TACoS 513 x 513, 1-row tails: blk long (Lk > 128, Lq >= 128) / blk long (Lk > 128)
    (6, 4, 140, 200, 32, 32, 3, 2),    # blk long / blk long
    (4, 4, 7, 300, 32, 32, 2, 1),      # lane-per-key (Lk > 128, Lq < 128) / blk long
    (4, 8, 112, 112, 32, 32, 2, 1),    # blk short / lane-per-key (staged head beyond 64 KB LDS; several key tiles, ADDS
                                       # into dq; in a phase the lane-per-key group kernel)
    (4, 8, 200, 40, 32, 32, 2, 1),     # blk short / lane-per-key, one key tile (writes dq; in a phase its group kernel)
    (6, 4, 50, 60, 64, 32, 3, 2),      # blk dk 64 packed (Lq > 16) / blk dk 64 packed
    (6, 4, 20, 12, 8, 8, 3, 2),        # lane-per-key (dk 8) / lane-per-key, one key tile
    (6, 4, 9, 300, 16, 16, 3, 2),      # lane-per-key (dk 16) / lane-per-key, several key tiles
]
# mask_group alone, mask_mod alone (one padded batch), both (stacked passes of a padded batch), both with n = 1
QUIRK_MODES = [("group", True, None, 0.0), ("mod", False, "n", 0.1), ("group+mod", True, "n", 0.1),
               ("group+mod1", True, 1, 0.0)]


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "phase"])
@pytest.mark.parametrize("mode,use_group,use_mod,drop_p", QUIRK_MODES, ids=[m[0] for m in QUIRK_MODES])
@pytest.mark.parametrize("B,H,Lq,Lk,dk,dv,G,n", QUIRK_CASES)
def test_quirk_group_and_modulus(B, H, Lq, Lk, dk, dv, G, n, mode, use_group, use_mod, drop_p, grouped):
    group = G if use_group else 0
    mod = n if use_mod == "n" else use_mod

    def make(s):
        kpad, qpad = make_pad(B, Lk, 10 + s), make_pad(B, Lq, 11 + s)
        return Problem(20 + s, B, H, Lq, Lk, dk, dv, quirk_mask(qpad, kpad, H, group=group, mod=mod), kpad=kpad,
                       qpad=qpad, group=group, drop_p=drop_p)

    probs = copies(grouped, make)
    fw, gs = run(probs, grouped, mod=mod)
    tag = "quirk-%s-%s" % (mode, "x".join(map(str, (B, H, Lq, Lk, dk, dv))))
    for p, (o, lse), g in zip(probs, fw, gs):
        check_fwd(p, o, lse, tag)
        check_bwd(p, o, lse, g, tag)


# ------------------------------------------------------------------------------------------ split heads (decoder), k_add
SPLIT_CASES = [
    # B, H, Lq, Lk (dk = 64 as [content || position] halves of 32, dv = 32)   forward family / backward family
    (32, 8, 10, 75),   # decoder self queries x video memory: lane-per-key (dk 64, Lq <= 16) / blk dk 64 split
    (32, 8, 40, 75),   # blk dk 64 split (Lq > 16) / blk dk 64 split
    (8, 8, 10, 513),   # C5 memory: lane-per-key (Lk > 128) / lane-per-key (staged head too large; ADDS into dq)
    (4, 8, 40, 513),   # lane-per-key / lane-per-key
]
SPLIT_MODES = [(None, 0.0), ("alias", 0.0), ("alias", 0.1), ("own", 0.1)]


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "phase"])
@pytest.mark.parametrize("k_add,drop_p", SPLIT_MODES, ids=["plain", "kadd_alias", "kadd_alias_drop", "kadd_own_drop"])
@pytest.mark.parametrize("B,H,Lq,Lk", SPLIT_CASES)
def test_split_heads_with_k_add(B, H, Lq, Lk, k_add, drop_p, grouped):
    def make(s):
        kpad = make_pad(B, Lk, 30 + s)  # mem_pad
        return Problem(40 + s, B, H, Lq, Lk, 64, 32, kpad_mask(kpad, H, Lq), kpad=kpad, drop_p=drop_p, split=k_add or "none")

    probs = copies(grouped, make)
    fw, gs = run(probs, grouped)
    tag = "split-%s-%g-%dx%d" % (k_add, drop_p, Lq, Lk)
    for p, (o, lse), g in zip(probs, fw, gs):
        check_fwd(p, o, lse, tag)
        check_bwd(p, o, lse, g, tag)


# -------------------------------------------------------------------------------------------------------------- causal
CAUSAL_CASES = [
    # B, H, L, dk, dv: every causal shape takes the lane-per-key forward (the other families refuse MESM_MASK_CAUSAL)
    (32, 8, 77, 64, 64),  # frozen CLIP text tower
    (3, 2, 19, 32, 32),   # small, ragged
    (5, 4, 13, 8, 8),
]


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "phase"])
@pytest.mark.parametrize("use_kpad", [False, True], ids=["nopad", "kpad"])
@pytest.mark.parametrize("B,H,L,dk,dv", CAUSAL_CASES)
def test_causal_forward(B, H, L, dk, dv, use_kpad, grouped):
    def make(s):
        kpad = make_pad(B, L, 50 + s) if use_kpad else None
        return Problem(60 + s, B, H, L, L, dk, dv, causal_mask(B, H, L, L, kpad), kpad=kpad, causal=True)

    probs = copies(grouped, make)
    fw, _ = run(probs, grouped, backward=False)
    for p, (o, lse) in zip(probs, fw):
        check_fwd(p, o, lse, "causal-%dx%d" % (L, dk))


def test_causal_backward_is_refused():
    """MESM_MASK_CAUSAL is forward only: mesm_attn_bwd and mesm_attn_bwd_group return an error and write nothing"""
    from mesm_amd import _lib
    from mesm_amd import kernels as kn
    B, H, L, dk = 2, 2, 9, 32
    p = Problem(70, B, H, L, L, dk, dk, causal_mask(B, H, L, L), causal=True)
    o, lse = p.fwd()
    g = [torch.full_like(t, float("nan")) for t in (p.q, p.k, p.v)]
    a = kn._attn_args(p.q, p.k, p.v, o, lse, H, None, None, p.scale, (0.0, 0), 0, True)
    a.d_o, a.dq, a.dk_, a.dv_ = p.do.data_ptr(), g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr()
    with pytest.raises(_lib.MesmError):
        kn.check(kn.lib().mesm_attn_bwd(ctypes.byref(a), kn.stream_ptr()), "mesm_attn_bwd")
    arr = (kn.AttnArgs * 2)(a, a)
    with pytest.raises(_lib.MesmError):
        kn.check(kn.lib().mesm_attn_bwd_group(arr, 2, kn.stream_ptr()), "mesm_attn_bwd_group")
    torch.cuda.synchronize()
    assert all(bool(t.isnan().all()) for t in g)


# -------------------------------------------------------------------------------------------------- fully masked rows
FULL_CASES = [
    # B, H, Lq, Lk, dk, dv, quirk, split        forward family
    (8, 4, 20, 30, 32, 32, True, None),        # blk short
    (4, 4, 140, 200, 32, 32, True, None),      # blk long
    (4, 4, 40, 60, 64, 32, False, None),       # blk dk 64 packed
    (4, 8, 40, 75, 64, 32, False, "alias"),    # blk dk 64 split, k_add
    (4, 8, 10, 75, 64, 32, False, "alias"),    # lane-per-key split (Lq <= 16), k_add
    (4, 4, 7, 300, 32, 32, True, None),        # lane-per-key (Lk > 128, Lq < 128)
    (6, 4, 20, 12, 8, 8, False, None),         # lane-per-key dk 8
    (6, 4, 9, 300, 16, 16, True, None),        # lane-per-key dk 16, several key tiles
]


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "phase"])
@pytest.mark.parametrize("B,H,Lq,Lk,dk,dv,quirk,split", FULL_CASES)
def test_rows_with_every_key_masked(B, H, Lq, Lk, dk, dv, quirk, split, grouped):
    """batch row 1 pads every key: its own rows are fully masked; under the quirk also the rows i with qpad[1, i] of
    every (b, h) whose mask row is 1.  Those rows give NaN and a non-finite lse, the others are unaffected."""
    def make(s):
        kpad = make_pad(B, Lk, 80 + s)
        kpad[1] = True
        if quirk:
            qpad = make_pad(B, Lq, 81 + s)
            qpad[1, ::3] = True
            return Problem(90 + s, B, H, Lq, Lk, dk, dv, quirk_mask(qpad, kpad, H), kpad=kpad, qpad=qpad)
        return Problem(90 + s, B, H, Lq, Lk, dk, dv, kpad_mask(kpad, H, Lq), kpad=kpad, split=split)

    probs = copies(grouped, make)
    fw, _ = run(probs, grouped, backward=False)
    for p, (o, lse) in zip(probs, fw):
        full = p.masked.all(-1)
        assert bool(full[1].all())
        if quirk:  # rows of other batch rows that the quirk sends to row 1's masks
            assert bool(full[torch.arange(B) != 1].any())
        check_fwd(p, o, lse, "full-%dx%dx%d" % (Lq, Lk, dk))
