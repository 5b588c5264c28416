"""float16 video features on the MI355X (mesm_amd.FEATURE_DTYPES): the half-input LayerNorm kernels against the float
kernels on the widened input -- widening is exact and the lanes, the loads' columns and the order of every sum are the
float kernel's, so y / mean / rstd must agree BIT FOR BIT --, a whole training / evaluation step on float16 features
against the same step on those features widened, and the three graph paths, which must never serve a batch of one
element type from a graph captured over the other.

Every test first asserts that the build knows float16 features: on a tree without them it fails there, on the host,
and no half buffer ever reaches a kernel that would read it as floats (twice the bytes: out of bounds).

The parameter-gradient backward adds its per-workgroup partial sums atomically (several row blocks per column, in
whatever order they finish), so dgamma / dbeta are not bit-reproducible even float against float: they are held to the
bound of tests/test_kernels_gpu.py::test_layernorm (its rel_err and TOL, imported) against fp64 and against the float
kernel."""
import argparse
import ctypes
import math

import numpy as np
import pytest
import torch

import mesm_amd

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN = float("nan")
# (rows, D): D % 4 = 2 (the shifted 16-byte path), odd (every shift 0..3), 1-wide, aligned 2-chunk, aligned narrow;
# no row count is a multiple of the 4 waves of a forward workgroup
PROBLEMS = [(203, 2818), (67, 4098), (131, 2817), (1027, 301), (1057, 512), (65, 300)]
DROPS = [(0.0, 0), (0.1, 3)]


def _feature_guard():
    assert torch.float16 in getattr(mesm_amd, "FEATURE_DTYPES", ())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, what):
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape, what
    assert bool(torch.isfinite(a).all()), what
    assert torch.equal(_bits(a), _bits(b)), (what, float((a - b).abs().max()))


def _half_problem(rows, D, seed, offset=64):
    """x (rows, D) float16 as a VIEW into the middle of a NaN-filled allocation, `offset` elements in (64: 128 bytes,
    8-byte aligned; 1: two bytes off) -- a read one element outside a row range poisons that row's mean.  Values: N(0.5, 2)
    plus +-0, float16 subnormals and +-65504 at the row ends and in the middle."""
    g = torch.Generator().manual_seed(seed)
    vals = (torch.randn(rows, D, generator=g) * 2.0 + 0.5).half()
    sub = torch.tensor([1, 3, 1023], dtype=torch.int16).view(torch.float16)  # subnormals: 2^-24, 3 * 2^-24, the largest
    special = torch.cat([torch.tensor([0.0, -0.0, 65504.0, -65504.0], dtype=torch.float16), sub, -sub])
    for j, v in enumerate(special):
        r = (7 * j) % rows
        for c in (0, 1, D // 2 + j, D - 2, D - 1):
            vals[(r + c) % rows, c] = v
    buf = torch.full((offset + rows * D + 64,), NAN, dtype=torch.float16, device=DEV)
    x = buf[offset:offset + rows * D].view(rows, D)
    x.copy_(vals.to(DEV))
    gam = (torch.randn(D, generator=g) * 0.2 + 1.0).to(DEV)
    bet = (torch.randn(D, generator=g) * 0.1).to(DEV)
    return x, gam, bet


def _nan_out(rows, D):
    return torch.full((rows * D,), NAN, device=DEV)


# ----------------------------------------------------------------------------- kernels: forward
@pytest.mark.parametrize("drop", DROPS)
@pytest.mark.parametrize("rows,D", PROBLEMS)
def test_forward_is_bit_identical_to_the_float_kernel_on_the_widened_input(rows, D, drop):
    _feature_guard()
    from mesm_amd import kernels as kn
    x, g, b = _half_problem(rows, D, 40)
    assert x.data_ptr() % 8 == 0 and x.dtype == torch.float16
    y, mean, rstd = kn.layernorm_fwd(x, g, b, 1e-5, drop, out=_nan_out(rows, D))
    yf, meanf, rstdf = kn.layernorm_fwd(x.float(), g, b, 1e-5, drop, out=_nan_out(rows, D))
    torch.cuda.synchronize()
    assert y.dtype == mean.dtype == rstd.dtype == torch.float32 and y.shape == x.shape
    _same_bits(mean, meanf, "mean")
    _same_bits(rstd, rstdf, "rstd")
    _same_bits(y, yf, "y")
    if drop[0] == 0.0:  # and the float kernel itself is right on these values (fp64, the bound of test_layernorm)
        from test_kernels_gpu import TOL, rel_err
        ref = torch.nn.functional.layer_norm(x.double(), (D,), g.double(), b.double(), 1e-5)
        assert rel_err(y, ref) < TOL
    else:
        assert 0.02 < float((y == 0).float().mean()) < 0.25  # the mask was applied (p = 0.1)


@pytest.mark.parametrize("rows,D", PROBLEMS)
def test_forward_pairs_of_one_phase_are_bit_identical_twin_launch_included(rows, D):
    """three members of one kn.phase(): the same x under two dropout masks (D = 2818 / 4098: the twin launch, one read of
    x and two outputs) and another problem of the same width"""
    _feature_guard()
    from mesm_amd import kernels as kn
    x, g, b = _half_problem(rows, D, 41)
    x2, _, _ = _half_problem(rows + 3, D, 42)

    def run(xa, xb):
        with kn.phase():
            ra = kn.layernorm_fwd(xa, g, b, 1e-5, (0.1, 3), out=_nan_out(rows, D))
            rb = kn.layernorm_fwd(xa, g, b, 1e-5, (0.2, 5), out=_nan_out(rows, D))
            rc = kn.layernorm_fwd(xb, g, b, 1e-5, (0.0, 0), out=_nan_out(rows + 3, D))
        torch.cuda.synchronize()
        return ra, rb, rc

    half = run(x, x2)
    flt = run(x.float(), x2.float())
    for i, (h, f) in enumerate(zip(half, flt)):
        for name, th, tf in zip(("y", "mean", "rstd"), h, f):
            _same_bits(th, tf, (i, name))
    assert not torch.equal(half[0][0], half[1][0])  # two masks


def _raw_args(kn, x, g, b, y, mean, rstd):
    a = kn.LnArgs()
    a.x, a.gamma, a.beta, a.y, a.mean, a.rstd = (x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                                 rstd.data_ptr())
    a.rows, a.D, a.eps = x.shape[0], x.shape[1], 1e-5
    return a


@pytest.mark.parametrize("rows,D", [(203, 2818), (131, 2817), (65, 300)])
def test_a_view_two_bytes_off_is_ealign_and_the_wrapper_recovers(rows, D):
    _feature_guard()
    from mesm_amd import kernels as kn
    from mesm_amd._lib import lib, stream_ptr
    x, g, b = _half_problem(rows, D, 43, offset=65)
    assert x.data_ptr() % 8 == 2
    y = _nan_out(rows, D)
    mean, rstd = torch.full((rows,), NAN, device=DEV), torch.full((rows,), NAN, device=DEV)
    a = _raw_args(kn, x, g, b, y, mean, rstd)
    assert lib().mesm_layernorm_fwd_group_xh(ctypes.byref(a), 1, stream_ptr()) == -2  # MESM_EALIGN
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(mean).all())  # nothing was launched
    yf, meanf, rstdf = kn.layernorm_fwd(x.float(), g, b, 1e-5, (0.1, 3))
    got = kn.layernorm_fwd(x, g, b, 1e-5, (0.1, 3), out=y)
    with kn.phase():
        got_p = kn.layernorm_fwd(x, g, b, 1e-5, (0.1, 3), out=_nan_out(rows, D))
    torch.cuda.synchronize()
    for r in (got, got_p):
        _same_bits(r[0], yf, "y")
        _same_bits(r[1], meanf, "mean")
        _same_bits(r[2], rstdf, "rstd")


def test_the_half_entry_points_refuse_what_they_do_not_cover():
    _feature_guard()
    from mesm_amd import kernels as kn
    from mesm_amd._lib import lib, stream_ptr
    rows, D = 9, 2818
    x, g, b = _half_problem(rows, D, 44)
    y = _nan_out(rows, D)
    mean, rstd = torch.full((rows,), NAN, device=DEV), torch.full((rows,), NAN, device=DEV)
    dy, dg, db = torch.ones(rows, D, device=DEV), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    for field in ("add", "dx", "dx2", "dyb", "addend", "relu_in", "accumulate_dx"):
        a = _raw_args(kn, x, g, b, y, mean, rstd)
        a.dy, a.dgamma, a.dbeta = dy.data_ptr(), dg.data_ptr(), db.data_ptr()
        setattr(a, field, 1 if field in ("relu_in", "accumulate_dx") else y.data_ptr())
        assert lib().mesm_layernorm_fwd_group_xh(ctypes.byref(a), 1, stream_ptr()) == -1, field  # MESM_EINVAL
        assert lib().mesm_layernorm_bwd_group_xh(ctypes.byref(a), 1, stream_ptr()) == -1, field
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and float(dg.abs().sum()) == 0.0
    # the wrappers say it in words, before any launch
    m = torch.zeros(rows, device=DEV)
    with pytest.raises(TypeError, match="need_dx=False"):
        kn.layernorm_bwd(dy, x, g, m, m, dg, db)  # need_dx defaults to True
    with pytest.raises(TypeError, match="float32 or float16"):
        kn.layernorm_fwd(x.float().bfloat16(), g, b)
    with pytest.raises(TypeError, match="float32 or float16"):
        kn.layernorm_fwd(x.double(), g, b)
    with pytest.raises(TypeError, match="gamma must be float32"):
        kn.layernorm_fwd(x, g.half(), b)
    with pytest.raises(TypeError, match="add"):
        kn.layernorm_fwd(x, g, b, add=torch.zeros(rows, D, device=DEV))
    with pytest.raises(TypeError, match="dy must be float32"):
        kn.layernorm_bwd(dy.half(), x, g, m, m, dg, db, need_dx=False)


# ----------------------------------------------------------------------------- kernels: parameter gradients
@pytest.mark.parametrize("drop", DROPS)
@pytest.mark.parametrize("rows,D", PROBLEMS)
def test_parameter_gradients_single_and_twin(rows, D, drop):
    """dgamma / dbeta from float16 x, alone and as two problems of one phase over the same x (the twin launch for D > 512),
    against the float kernel on the widened x and -- without dropout -- against fp64"""
    _feature_guard()
    from mesm_amd import kernels as kn
    from test_kernels_gpu import TOL, rel_err
    x, g, b = _half_problem(rows, D, 45)
    xf = x.float()
    _, mean, rstd = kn.layernorm_fwd(x, g, b)
    gen = torch.Generator().manual_seed(46)
    dy1, dy2 = (torch.randn(rows, D, generator=gen).to(DEV) for _ in range(2))
    drop2 = (drop[0], drop[1] + 4) if drop[0] else drop

    def single(xx):
        dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
        assert kn.layernorm_bwd(dy1, xx, g, mean, rstd, dg, db, need_dx=False, drop=drop) is None
        return dg, db

    def twin(xx):
        dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
        with kn.phase():
            kn.layernorm_bwd(dy1, xx, g, mean, rstd, dg, db, need_dx=False, drop=drop)
            kn.layernorm_bwd(dy2, xx, g, mean, rstd, dg, db, need_dx=False, drop=drop2)
        return dg, db

    for form, dys in ((single, dy1), (twin, dy1 + dy2)):
        (dgh, dbh), (dgf, dbf) = form(x), form(xf)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(dgh).all()) and bool(torch.isfinite(dbh).all())
        assert rel_err(dgh, dgf) < TOL and rel_err(dbh, dbf) < TOL, form.__name__
        if drop[0] == 0.0:
            xhat = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
            assert rel_err(dgh, (dys.double() * xhat).sum(0)) < TOL, form.__name__
            assert rel_err(dbh, dys.double().sum(0)) < TOL, form.__name__


# ----------------------------------------------------------------------------- the model, eager
def _build(workload, dropout, seed=7, train=True, auto=None, **auto_kw):
    from mesm_amd import build_criterion, build_model, synthetic
    args = synthetic.make_args(workload, device="cuda:0")
    torch.manual_seed(seed)
    model = build_model(args)
    crit = build_criterion(args)
    if not dropout:
        for m in model.modules():
            if hasattr(m, "p"):
                m.p = 0.0
    model.train(train)
    crit.train(train)
    if auto is not None:
        model.autograph(auto, **auto_kw)
    return args, model, crit


def _tensors(tree, prefix=""):
    """every tensor of an output dict, aux_outputs included -> {dotted name: tensor}"""
    out = {}
    for k, v in (tree.items() if isinstance(tree, dict) else enumerate(tree)):
        name = "%s%s" % (prefix, k)
        if torch.is_tensor(v):
            out[name] = v
        elif isinstance(v, (dict, list, tuple)):
            out.update(_tensors(v, name + "."))
    return out


def _train_step(model, crit, batch, name, neg, mw, step):
    model._step = step  # the dropout seeds of a step derive from it
    out = model(**batch, dataset_name=name, is_training=True, neg_index=neg, masked_words=mw)
    losses, total = crit(out, batch, True)
    model.zero_grad(set_to_none=True)
    total.backward()
    torch.cuda.synchronize()
    return ({k: v.detach().clone() for k, v in _tensors(out).items()}, {k: float(v) for k, v in losses.items()},
            float(total.detach()), model.gradbuf().flat.clone())


@pytest.mark.parametrize("workload,ragged", [("C2", False), ("C3a", False), ("C3b", False), ("C5", False), ("C3a", True)])
def test_a_training_step_on_float16_features_is_the_step_on_the_widened_features(workload, ragged, deterministic_forward):
    """train mode, dropout on: A = the model on vf.half().float(), B = the same weights, step counter and draws on vf.half().
    Every output and loss entry bit-identical; gradients within the eager-versus-replay bound of tests/test_autograph_gpu.py
    under this fixture (1e-4 of the gradient norm: the backward's atomic sums are not ordered)."""
    _feature_guard()
    from mesm_amd import synthetic
    args, model, crit = _build(workload, dropout=True)
    host = synthetic.workload_batch(workload, seed=11, ragged=ragged)
    neg, mw = synthetic.host_draws(host, seed=11)
    half = synthetic.to_device(host, DEV)
    half["video_feat"] = half["video_feat"].half()
    wide = dict(half, video_feat=half["video_feat"].float())
    out_a, ls_a, tot_a, flat_a = _train_step(model, crit, wide, args.dataset_name, neg, mw, 100)
    out_b, ls_b, tot_b, flat_b = _train_step(model, crit, half, args.dataset_name, neg, mw, 100)
    assert set(out_a) == set(out_b) and len(out_a) > 8
    for k, a in out_a.items():
        b = out_b[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert torch.equal(a, b) and (not a.dtype.is_floating_point or torch.equal(_bits(a.float()), _bits(b.float()))), k
    assert ls_a == ls_b and tot_a == tot_b and math.isfinite(tot_a)
    assert float((flat_a - flat_b).norm()) / max(float(flat_a.norm()), 1e-6) < 1e-4
    # dropout was on: another step counter gives another step
    _, _, tot_c, _ = _train_step(model, crit, half, args.dataset_name, neg, mw, 101)
    assert tot_c != tot_b


@pytest.mark.parametrize("workload", ["C3a", "C3b"])
def test_evaluation_rows_from_float16_features_equal_those_from_the_widened_features(workload, deterministic_forward):
    _feature_guard()
    from mesm_amd import synthetic
    from mesm_amd.postprocess import compute_mr_results
    args, model, crit = _build(workload, dropout=True, train=False)
    opt = argparse.Namespace(dataset_name=args.dataset_name, clip_len=2, max_ts_val=150, sort_results=True)
    res = []
    for dt in (torch.float32, torch.float16):
        stream = []
        for i in range(2):
            b = synthetic.to_device(synthetic.workload_batch(workload, seed=30 + i, ragged=True), DEV)
            b["video_feat"] = b["video_feat"].half().to(dt)
            n = b["video_feat"].shape[0]
            b["qid"], b["sentence"], b["video_id"] = list(range(n)), ["q%d" % j for j in range(n)], ["v%d" % j for j in range(n)]
            stream.append(b)
        torch.manual_seed(3)
        np.random.seed(3)
        res.append(compute_mr_results(model, stream, opt, criterion=crit))
    (rows_a, meters_a), (rows_b, meters_b) = res
    assert len(rows_a) == len(rows_b) > 0
    for ra, rb in zip(rows_a, rows_b):
        assert ra == rb  # qid, windows and the saliency lists
    assert meters_a == meters_b


def test_float16_step_against_the_cpu_oracle_on_the_widened_features():
    """C3a at full size as tests/test_model_gpu.py::test_full_size_workload_against_cpu_oracle runs it (its helpers and
    bounds), the device side on float16 features, the oracle on those features widened"""
    _feature_guard()
    from mesm_amd import build_criterion, build_model, synthetic
    from oracle import mesm_oracle as O
    from test_model_gpu import TOL, rel, run_step
    args = synthetic.make_args("C3a", device="cuda:0")
    torch.manual_seed(1234)
    model = build_model(args)
    crit = build_criterion(args)
    batch = synthetic.workload_batch("C3a", seed=0, feature_dtype=torch.float16)
    neg, masked = synthetic.host_draws(batch, seed=0)
    out, losses, total = run_step(model, crit, batch, vars(args), neg, masked)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    wide = dict(batch, video_feat=batch["video_feat"].float())
    o_out, o_losses, o_total, o_grads, o_idx = O.train_step(sd, dict(vars(args)), wide, neg, masked)
    for k in ("pred_logits", "pred_spans", "saliency_scores", "neg_saliency_scores", "recfw_words_logit"):
        assert rel(out[k], o_out[k]) < TOL, k
    for k, v in o_losses.items():
        assert abs(float(losses[k]) - float(v)) < TOL * max(1.0, abs(float(v))), k
    assert abs(float(total) - float(o_total)) < TOL * max(1.0, abs(float(o_total)))
    worst = 0.0
    for n, p in model.named_parameters():
        if n in o_grads:
            a, b = p.grad.detach().double().cpu(), o_grads[n].double()
            worst = max(worst, float((a - b).norm()) / max(float(b.norm()), 1e-3 * b.numel() ** 0.5))
    assert worst < 1e-2, worst


def test_the_model_refuses_feature_types_it_would_misread():
    _feature_guard()
    from mesm_amd import synthetic
    args, model, crit = _build("C3b", dropout=False)
    batch = synthetic.to_device(synthetic.workload_batch("C3b", seed=1), DEV)
    neg, mw = synthetic.host_draws(synthetic.workload_batch("C3b", seed=1), seed=1)
    kw = dict(dataset_name=args.dataset_name, is_training=True, neg_index=neg, masked_words=mw)
    step = model._step
    for bad in (torch.bfloat16, torch.float64):
        with pytest.raises(TypeError, match="float32 or float16"):
            model(**dict(batch, video_feat=batch["video_feat"].to(bad)), **kw)
    with pytest.raises(TypeError, match="words_id"):
        model(**dict(batch, words_id=batch["words_id"].half()), **kw)
    assert model._step == step  # refused before the step began: no launch


# ----------------------------------------------------------------------------- graph paths
def test_step_cache_captures_float16_steps_from_host_batches_and_keeps_the_types_apart(deterministic_forward):
    _feature_guard()
    from mesm_amd import synthetic
    from mesm_amd.graphed import StepCache
    from test_autograph_gpu import _eager_on
    args, model, crit = _build("C3a", dropout=False)
    name = args.dataset_name
    cache = StepCache(model, crit, name)
    hb = [synthetic.workload_batch("C3a", seed=20 + i, feature_dtype=torch.float16) for i in range(3)]
    _, gs = cache.run(hb[0])
    assert gs.batch["video_feat"].dtype == torch.float16 and gs.batch["video_feat"].is_cuda
    for b in hb[1:]:
        total_g, gs2 = cache.run(b)
        torch.cuda.synchronize()
        assert gs2 is gs
        total_g, flat_g = float(total_g), model.gradbuf().flat.clone()
        neg, mw = gs._draws
        _, _, total_e, flat_e = _eager_on(model, crit, synthetic.to_device(b, DEV), name, neg, mw)
        assert abs(total_e - total_g) < 1e-5 * max(1.0, abs(total_e)), (total_e, total_g)
        assert float((flat_e - flat_g).norm()) / max(float(flat_e.norm()), 1e-6) < 1e-4
    assert (cache.captures, cache.replays) == (1, 2)
    # a float32 batch does not fit the float16 step (copy_ would convert it on the way in) ...
    f32 = synthetic.workload_batch("C3a", seed=22)
    with pytest.raises(ValueError, match="dtype"):
        gs.load_batch(f32, redraw=True)
    # ... which still serves float16 batches, and the cache gives the float32 batch a graph of its own
    gs.load_batch(hb[1], redraw=True)
    total_f, gs_f = cache.run(f32)
    assert gs_f is not gs and gs_f.batch["video_feat"].dtype == torch.float32 and cache.captures == 2
    # same values (the float16 features widened are not the float32 draw, so only the float16 pair is comparable)
    wide = dict(hb[2], video_feat=hb[2]["video_feat"].float())
    total_w, gs_w = cache.run(wide)
    assert gs_w is gs_f
    torch.cuda.synchronize()
    flat_w = model.gradbuf().flat.clone()
    neg, mw = gs_f._draws
    _, _, total_e, flat_e = _eager_on(model, crit, synthetic.to_device(hb[2], DEV), name, neg, mw)
    assert abs(total_e - float(total_w)) < 1e-5 * max(1.0, abs(total_e))
    assert float((flat_e - flat_w).norm()) / max(float(flat_e.norm()), 1e-6) < 1e-4
    with pytest.raises(ValueError, match="dtype"):
        gs_f.load_batch(hb[0], redraw=True)


def test_autograph_gives_each_feature_type_its_own_graph_and_alternates_correctly(deterministic_forward):
    _feature_guard()
    from mesm_amd import synthetic
    from test_autograph_gpu import _eager_on
    args, model, crit = _build("C3a", dropout=False, auto=True)
    name, auto = args.dataset_name, model._auto
    replayed = []
    for i in range(6):
        dt = torch.float16 if i % 2 == 0 else torch.float32
        batch = synthetic.to_device(synthetic.workload_batch("C3a", seed=50 + i, feature_dtype=dt), DEV)
        out = model(**batch, dataset_name=name, is_training=True)
        losses, total = crit(out, batch, True)
        model.zero_grad(set_to_none=True)
        total.backward()
        torch.cuda.synchronize()
        step = out._auto_step
        replayed.append(step is not None)
        if step is None:
            continue
        assert step.batch["video_feat"].dtype == dt
        total_g, flat_g = float(total.detach()), model.gradbuf().flat.clone()
        neg, mw = step._draws
        _, _, total_e, flat_e = _eager_on(model, crit, batch, name, neg, mw)
        assert abs(total_e - total_g) < 1e-5 * max(1.0, abs(total_e)), (i, total_e, total_g)
        assert float((flat_e - flat_g).norm()) / max(float(flat_e.norm()), 1e-6) < 1e-4, i
    # per type: the first visit runs eagerly, the second captures its graph and replays it, the third replays
    assert replayed == [False, False, True, True, True, True]
    assert (auto.eager, auto.captures, auto.replays) == (2, 2, 4)


def test_autograph_eval_replays_float16_batches_from_their_own_graph(deterministic_forward):
    _feature_guard()
    from mesm_amd import synthetic
    from test_eval_graph_gpu import _compare, _compare_losses, _eval_call, _seeded
    args, model, crit = _build("C3a", dropout=False, train=False, auto=True, eval=True)
    name, auto = args.dataset_name, model._auto
    for i in range(6):
        dt = torch.float16 if i % 2 == 0 else torch.float32
        b = synthetic.to_device(synthetic.workload_batch("C3a", seed=70 + i, feature_dtype=dt), DEV)
        _seeded(900 + i)
        out_r, res_r = _eval_call(model, crit, b, name)
        model.autograph(eval=False)
        _seeded(900 + i)
        out_e, res_e = _eval_call(model, crit, b, name)
        model.autograph(eval=True)
        _compare(out_r, out_e)
        _compare_losses(res_r, res_e)
    assert (auto.eval_eager, auto.eval_captures, auto.eval_replays) == (2, 2, 4)
    assert (auto.captures, auto.replays) == (0, 0)
