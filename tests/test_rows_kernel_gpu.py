"""postprocess.device_rows (mesm_windows_rows: ranking, 4-decimal rounding, clamp and clip-grid snap on the device)
against postprocess.predict_windows, the host referee: the rows must be EXACTLY equal, signs of zero included."""
import ctypes
import math

import pytest
import torch

from io_cases import MR_CASES, mr_inputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _bits(rows):
    return [[[(x, math.copysign(1.0, x)) for x in r] for r in q] for q in rows]


def _check(lg, sp, du, **kw):
    from mesm_amd.postprocess import device_rows, predict_windows
    sort = kw.pop("sort_results", True)
    got = device_rows(lg, sp, du, sort_results=sort, **kw)
    assert got.dtype == torch.float64 and tuple(got.shape) == tuple(lg.shape[:2]) + (3,)
    want = predict_windows(lg, sp, du, sort_results=sort, **kw)
    g = got.tolist()
    assert g == want
    assert _bits(g) == _bits(want)


@pytest.mark.parametrize("name", sorted(MR_CASES))
def test_golden_mr_cases(name):
    c = MR_CASES[name]
    _, outs = mr_inputs(c)
    loader, _ = mr_inputs(c)
    for b, o in zip(loader, outs):
        _check(o["pred_logits"].to(DEV), o["pred_spans"].to(DEV), b["duration"].to(DEV), clip_len=c["clip_len"])


def _random(N, Q, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(N, Q, 2, generator=g) * scale
    sp = torch.rand(N, Q, 2, generator=g)
    sp[..., 1] = sp[..., 1] * 0.6 + 0.001
    du = torch.rand(N, generator=g) * 150 + 10
    return lg.to(DEV), sp.to(DEV), du.to(DEV)


@pytest.mark.parametrize("clip_len", [-1, 1, 2])
@pytest.mark.parametrize("Q", [1, 10, 64])
def test_random_queries(clip_len, Q):
    N = 4000 if Q == 10 else 600
    _check(*_random(N, Q, 100 + Q + clip_len), clip_len=clip_len)


@pytest.mark.parametrize("clip_len", [-1, 2])
def test_unsorted(clip_len):
    _check(*_random(500, 10, 7), clip_len=clip_len, sort_results=False)


def test_ties_clamps_and_negative_starts():
    N, Q = 300, 10
    g = torch.Generator().manual_seed(3)
    # tied scores: only a few distinct logit pairs per query -> equal softmax scores, the stable order decides
    base = torch.randn(N, 3, 2, generator=g)
    pick = torch.randint(0, 3, (N, Q), generator=g)
    lg = torch.gather(base, 1, pick[..., None].expand(N, Q, 2)).contiguous()
    # centres / widths that give windows beyond both clamp bounds and negative starts
    sp = torch.rand(N, Q, 2, generator=g) * 1.6 - 0.3
    du = torch.rand(N, generator=g) * 200 + 50
    _check(lg.to(DEV), sp.to(DEV), du.to(DEV), clip_len=2, max_ts_val=150)
    _check(lg.to(DEV), sp.to(DEV), du.to(DEV), clip_len=-1, max_ts_val=150)
    # window ends that are exact decimal ties (k / 32) and tiny negatives that round to -0.0: duration 1, width 0
    k = torch.arange(N * Q, dtype=torch.float32).reshape(N, Q) * 2 + 1
    cx = torch.where(torch.arange(Q) % 2 == 0, k / 32.0 / 160.0, torch.full((N, Q), -1e-5))
    sp2 = torch.stack([cx, torch.zeros_like(cx)], -1)
    du2 = torch.ones(N) * 160.0
    _check(lg.to(DEV), sp2.to(DEV), du2.to(DEV), clip_len=-1, min_ts_val=-1e9, max_ts_val=1e9)
    _check(lg.to(DEV), sp2.to(DEV), du2.to(DEV), clip_len=1)


@pytest.mark.parametrize("clip_len", [-1, 2])
def test_starts_that_round_to_negative_zero_keep_their_sign_through_the_clamp(clip_len):
    """a start in (-5e-5, 0) rounds to -0.0; np.clip / torch.clamp against min_ts_val = 0 keep it, and so must the kernel"""
    N, Q = 64, 10
    g = torch.Generator().manual_seed(9)
    lg = torch.randn(N, Q, 2, generator=g)
    cx = torch.where(torch.arange(Q) % 2 == 0, torch.full((N, Q), -1e-7), torch.full((N, Q), 0.1))
    w = torch.where(torch.arange(Q) % 2 == 0, torch.zeros(N, Q), torch.full((N, Q), 0.2 + 2e-7))
    sp = torch.stack([cx, w], -1)
    du = torch.full((N,), 160.0)
    _check(lg.to(DEV), sp.to(DEV), du.to(DEV), clip_len=clip_len)  # default min_ts_val = 0, max_ts_val = 150
    from mesm_amd.postprocess import device_rows
    got = device_rows(lg.to(DEV), sp.to(DEV), du.to(DEV), clip_len=clip_len).cpu()
    assert bool(torch.signbit(got[..., 0]).any())  # the case is really met


def test_more_than_64_queries_is_refused():
    from mesm_amd import _lib
    from mesm_amd.postprocess import device_rows
    lg, sp, du = _random(2, 65, 1)
    out = torch.empty(2, 65, 3, dtype=torch.float64, device=DEV)
    rc = _lib.lib().mesm_windows_rows(_lib.ptr(lg), _lib.ptr(sp), _lib.ptr(du), _lib.ptr(out), 2, 65, 2.0, 0.0, 150.0, 1,
                                      _lib.stream_ptr())
    assert rc == -1  # MESM_EINVAL
    with pytest.raises(_lib.MesmError):
        device_rows(lg, sp, du)
