"""The fp64 attention reference of tests/attn_ref.py, on the CPU: its group / modulus masks are the oracle's T2V mask
applied per group or to the first n rows (and agree with the header's index rule), and its core reproduces
oracle.mesm_oracle.attention_core."""
import pytest
import torch

from attn_ref import attention, interleave, quirk_mask, row_bounds, split
from oracle import mesm_oracle as mo
from oracle.mesm_oracle import t2v_mask


def rand_pads(B, Lq, Lk, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, Lq, generator=g) < 0.4, torch.rand(B, Lk, generator=g) < 0.4


@pytest.mark.parametrize("B,H,G,n", [(8, 4, 0, None), (12, 8, 4, None), (12, 8, 0, 5), (12, 8, 6, 1), (64, 8, 32, 17),
                                     (9, 3, 3, 2)])
def test_quirk_mask_is_t2v_mask_per_group_of_the_first_n_rows(B, H, G, n):
    Lq, Lk = 7, 5
    qpad, kpad = rand_pads(B, Lq, Lk, B * 100 + G)
    m = quirk_mask(qpad, kpad, H, group=G, mod=n)
    assert m.shape == (B, H, Lq, Lk)
    stride = G or B
    nn = stride if n is None else n
    for s in range(0, B, stride):
        assert torch.equal(m[s:s + nn], t2v_mask(qpad[s:s + nn], kpad[s:s + nn], H))
        for b in range(s + nn, s + stride):  # dummy rows: their own key padding only
            assert torch.equal(m[b], kpad[b][None, None, :].expand(H, Lq, Lk))
    # the rule MesmAttnArgs documents: b2 = (b / G) G + ((b % G) H + h) mod n inside the group's first n rows
    for b in range(B):
        for h in range(H):
            bl = b % stride
            b2 = b - bl + ((bl * H + h) % nn if bl < nn else bl)
            want = kpad[b][None, :] | (qpad[b2][:, None] & kpad[b2][None, :])
            assert torch.equal(m[b, h], want), (b, h)


@pytest.mark.parametrize("quirk", [False, True])
def test_attention_reproduces_the_oracle_core(quirk):
    assert mo.DROPOUT is None  # the oracle's attention-probability dropout is off
    B, H, Lq, Lk, dk, dv = 6, 4, 9, 11, 8, 5
    g = torch.Generator().manual_seed(3)
    q, k = torch.randn(B, Lq, H * dk, generator=g), torch.randn(B, Lk, H * dk, generator=g)
    v = torch.randn(B, Lk, H * dv, generator=g)
    qpad, kpad = rand_pads(B, Lq, Lk, 4)
    kpad[:, 0] = False
    masked = quirk_mask(qpad, kpad, H) if quirk else kpad[:, None, None, :].expand(B, H, Lq, Lk)
    scale = dk ** -0.5
    o, lse = attention(q, k, v, H, masked, scale)
    ref = mo.attention_core(q.double(), k.double(), v.double(), H, masked, scale)
    assert torch.allclose(o, ref, rtol=1e-12, atol=1e-12)
    s = scale * torch.einsum("bqhd,bkhd->bhqk", q.double().view(B, Lq, H, dk), k.double().view(B, Lk, H, dk))
    s = s.masked_fill(masked, float("-inf"))
    assert torch.allclose(lse, torch.log(torch.exp(s).sum(-1)), rtol=1e-12, atol=1e-12)
    # a row whose keys are all masked: NaN output, -inf log-sum-exp
    masked = masked.clone()
    masked[1, 2, 3] = True
    o, lse = attention(q, k, v, H, masked, scale)
    assert torch.isnan(o[1, 3, 2 * dv:3 * dv]).all() and lse[1, 2, 3] == float("-inf")
    assert torch.isfinite(o[1, 3, :2 * dv]).all() and torch.isfinite(lse).sum() == lse.numel() - 1


def test_interleave_split_and_bounds_shapes():
    B, H, L, E = 2, 4, 3, 8
    a, b = torch.randn(B, L, E), torch.randn(B, L, E)
    x = interleave(a, b, H)
    assert torch.equal(x.view(B, L, H, 4)[..., :2], a.view(B, L, H, 2))
    a2, b2 = split(x, H)
    assert torch.equal(a2, a) and torch.equal(b2, b)
    q, k, v, do = torch.randn(B, 5, 16), torch.randn(B, 6, 16), torch.randn(B, 6, 8), torch.randn(B, 5, 8)
    masked = torch.zeros(B, H, 5, 6, dtype=torch.bool)
    bd = row_bounds(q, k, v, H, masked, 0.5, do=do)
    assert bd["o"].shape == bd["lse"].shape == bd["dq"].shape == (B, H, 5)
    assert bd["dk"].shape == bd["dv"].shape == (B, H, 6)
    assert all(bool((t > 0).all()) for t in bd.values())
