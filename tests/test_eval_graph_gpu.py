"""Evaluation calls on graph replays (mesm_amd/autograph.py, graphed.EvalGraphedStep), behind the reference's unchanged
eval.py:63,102 calls:

    model.eval(); with torch.no_grad():
        outputs = model(**batch, dataset_name=..., is_training=False)
        loss_dict, loss = criterion(outputs, batch, is_training=False)

opt-in only (model.autograph(eval=True)): the golden fixtures of the reference through a replay, replay against eager at
exact extents and in padded buckets, caller-owned outputs, the global RNG streams, training graphs untouched by an
evaluation epoch, and compute_mr_results with the opt-in against without."""
import argparse

import numpy as np
import pytest
import torch

from golden_io import CASES, EvalFixture, Fixture

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-3)


def _no_dropout(model):
    for m in model.modules():
        if hasattr(m, "p"):
            m.p = 0.0


def _build(workload="C3a", seed=7, **auto):
    from mesm_amd import build_criterion, build_model, synthetic
    args = synthetic.make_args(workload, device="cuda:0")
    torch.manual_seed(seed)
    model = build_model(args)
    crit = build_criterion(args)
    _no_dropout(model)
    model.eval()
    crit.eval()
    model.autograph(True, **auto)
    return args, model, crit


def _ragged(groups, seed, ids=0, Lv=None, Lw=None):
    from mesm_amd import synthetic
    w = synthetic.WORKLOADS["C3a"]
    b = synthetic.make_batch(w["dataset_name"], groups, Lv or w["Lv"], Lw or w["Lw"], w["v_feat_dim"], w["t_feat_dim"],
                             w["vocab_size"] + 1, seed=seed, ragged=True)
    n = sum(groups)
    b = synthetic.to_device(b, DEV)
    b["qid"] = list(range(ids, ids + n))
    b["sentence"] = ["q%d" % i for i in range(ids, ids + n)]
    b["video_id"] = ["v%d" % i for i in range(ids, ids + n)]
    return b


def _eval_call(model, crit, batch, name, with_crit=True):
    with torch.no_grad():
        out = model(**batch, dataset_name=name, is_training=False)
        res = crit(out, batch, is_training=False) if with_crit else None
    return out, res


def _seeded(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)


def _compare(out_r, out_e, tol=1e-4):
    assert set(out_r) == set(out_e)
    for k, e in out_e.items():
        if isinstance(e, list):
            assert len(out_r[k]) == len(e)
            pairs = [(out_r[k][i][kk], e[i][kk], k + "." + kk) for i in range(len(e)) for kk in e[i]]
        else:
            pairs = [(out_r[k], e, k)]
        for r, ee, name in pairs:
            assert tuple(r.shape) == tuple(ee.shape), (name, tuple(r.shape), tuple(ee.shape))
            if ee.dtype == torch.bool:
                assert torch.equal(r, ee), name
            else:
                assert rel(r, ee) < tol, (name, rel(r, ee))


def _compare_losses(res_r, res_e, tol=1e-4):
    (lr, tr), (le, te) = res_r, res_e
    assert set(lr) == set(le)
    for k in le:
        assert abs(float(lr[k]) - float(le[k])) < tol * max(1.0, abs(float(le[k]))), k
    assert abs(float(tr) - float(te)) < tol * max(1.0, abs(float(te)))


# ----------------------------------------------------------------------------- golden fixtures of the reference
@pytest.mark.parametrize("case", CASES)
def test_replayed_eval_call_matches_reference_golden(case, monkeypatch):
    from mesm_amd import build_criterion, build_model, draws, synthetic
    fx, ev = Fixture(case), EvalFixture(case)
    args = argparse.Namespace(**fx.cfg)
    args.device = "cuda:0"
    model = build_model(args)
    model.load_state_dict(fx.sd)
    crit = build_criterion(args)
    model.eval()
    crit.eval()
    model.autograph(True, eval=True)
    # the fixture's recorded negative draw stands in for the global stream (eager and replayed calls alike)
    monkeypatch.setattr(draws, "neg_index", lambda groups, n_valid=None, mode=None: ev.neg_index.numpy().copy())
    batch = synthetic.to_device(fx.batch, DEV)
    auto = model._auto
    for i in range(2):
        out, (losses, total) = _eval_call(model, crit, batch, fx.cfg["dataset_name"])
    assert auto.eval_replays >= 1 and auto.eval_captures == 1
    assert out._eval_losses is not None
    assert sorted(out.keys()) == ev.keys
    for k, v in ev.out.items():
        got = out["aux_outputs"][0][k[5:]] if k.startswith("aux0.") else out[k]
        if v.dtype == torch.bool:
            assert torch.equal(got.cpu(), v), k
        else:
            assert rel(got, v) < TOL, k
    assert set(losses) | {"total"} == set(ev.losses)
    for k, v in ev.losses.items():
        got = float(total) if k == "total" else float(losses[k])
        assert abs(got - v) < TOL * max(1.0, abs(v)), (k, got, v)


# ----------------------------------------------------------------------------- replay against eager
def test_replay_equals_eager_at_exact_extents(deterministic_forward):
    from mesm_amd import synthetic
    args, model, crit = _build(eval=True)
    name = args.dataset_name
    auto = model._auto
    batches = [synthetic.to_device(synthetic.workload_batch("C3a", seed=90 + i), DEV) for i in range(3)]
    for i, b in enumerate(batches):
        _seeded(500 + i)
        out_r, res_r = _eval_call(model, crit, b, name)
        if i == 0:
            assert out_r._eval_losses is None
            continue
        assert out_r._eval_losses is not None
        model.autograph(eval=False)
        _seeded(500 + i)
        out_e, res_e = _eval_call(model, crit, b, name)
        model.autograph(eval=True)
        _compare(out_r, out_e)
        _compare_losses(res_r, res_e)
    assert (auto.eval_eager, auto.eval_captures, auto.eval_replays) == (1, 1, 2)
    assert (auto.captures, auto.replays) == (0, 0)


def test_replay_equals_eager_in_padded_buckets(deterministic_forward):
    args, model, crit = _build(eval=True, pad=(75, 32), pairs=8)
    name = args.dataset_name
    auto = model._auto
    shapes = [[3, 4, 2, 5, 1, 3, 4, 2, 5, 1, 4, 3, 4], [4, 4, 2, 5, 1, 3, 4, 2, 5, 3, 4, 3, 3], [5, 4, 2, 5, 1, 3, 4, 2, 5, 3, 4, 3, 5]]
    for i, groups in enumerate(shapes):
        # clip / word extents below the bucket's (75, 32), as a loader that pads to the batch's longest video / query
        # emits them: the outputs come back with the caller's extents
        Lv, Lw = [(None, None), (None, 24), (70, 20)][i]
        b = _ragged(groups, 60 + i, Lv=Lv, Lw=Lw)
        _seeded(700 + i)
        out_r, res_r = _eval_call(model, crit, b, name)
        model.autograph(eval=False)
        _seeded(700 + i)
        out_e, res_e = _eval_call(model, crit, b, name)
        model.autograph(eval=True)
        assert out_r["pred_spans"].shape[0] == sum(groups)
        if Lw is not None:
            assert out_r["projed_words_feat"].shape[1] == Lw and out_r["expanded_words_mask"].shape[1] == Lw + 1
        if Lv is not None:
            assert out_r["saliency_scores"].shape[1] == Lv
        _compare(out_r, out_e)
        _compare_losses(res_r, res_e)
        assert (out_r._eval_losses is not None) == (i >= 1)
    assert auto.eval_captures == 1 and auto.eval_replays == 2


def test_outputs_belong_to_the_caller(deterministic_forward):
    from mesm_amd import synthetic
    args, model, crit = _build(eval=True)
    name = args.dataset_name
    ba, bb = (synthetic.to_device(synthetic.workload_batch("C3a", seed=s), DEV) for s in (11, 12))
    _eval_call(model, crit, ba, name)
    out_a, (la, ta) = _eval_call(model, crit, ba, name)
    assert out_a._eval_losses is not None
    snap = {k: v.clone() for k, v in out_a.items() if torch.is_tensor(v)}
    snap_l = {k: float(v) for k, v in la.items()}
    out_b, _ = _eval_call(model, crit, bb, name)
    assert out_b._eval_losses is not None
    torch.cuda.synchronize()
    for k, v in snap.items():
        assert torch.equal(out_a[k], v), k
    assert {k: float(v) for k, v in la.items()} == snap_l
    # the criterion on A's outputs with A's batch: A's captured losses; with another batch: the eager criterion
    la2, ta2 = crit(out_a, ba, is_training=False)
    assert float(ta2) == float(ta)
    lx, tx = crit(out_a, bb, is_training=False)
    with torch.no_grad():
        le, te = crit._forward(dict(out_a), bb, False)
    assert abs(float(tx) - float(te)) < 1e-6 * max(1.0, abs(float(te)))


@pytest.mark.parametrize("mode", ["vectorized", "reference"])
def test_global_rng_streams_advance_like_eager_calls(mode, monkeypatch):
    from mesm_amd import draws
    monkeypatch.setattr(draws, "MODE", mode)
    args, model, crit = _build(eval=True, pad=(75, 32), pairs=8)
    name = args.dataset_name
    stream = [_ragged([3, 2, 4, 1, 5, 2, 3, 1, 2, 4, 3, 2], 200 + i) for i in range(4)]
    states = []
    for on in (True, False):
        model.autograph(eval=on)
        _seeded(77)
        for b in stream:
            _eval_call(model, crit, b, name)
        states.append((torch.get_rng_state(), np.random.get_state()[1].copy(), np.random.get_state()[2]))
    assert model._auto.eval_replays >= 2
    assert torch.equal(states[0][0], states[1][0])
    assert np.array_equal(states[0][1], states[1][1]) and states[0][2] == states[1][2]


# ----------------------------------------------------------------------------- training untouched
def test_training_graphs_survive_an_evaluation_epoch(deterministic_forward):
    from mesm_amd import synthetic
    args, model, crit = _build(eval=True, pad=(75, 32), pairs=8)
    name = args.dataset_name
    auto = model._auto
    tb = synthetic.to_device(synthetic.workload_batch("C3a", seed=300), DEV)

    def train_step():
        model.train()
        crit.train()
        _seeded(900)
        out = model(**tb, dataset_name=name, is_training=True)
        _, loss = crit(out, tb, is_training=True)
        model.zero_grad(set_to_none=True)
        loss.backward()
        torch.cuda.synchronize()
        return out._auto_step is not None, float(loss), model.gradbuf().flat.clone()

    train_step()
    train_step()
    r1, l1, g1 = train_step()
    assert r1 and auto.captures == 1 and auto.replays == 2
    model.eval()
    crit.eval()
    for i in range(6):
        _eval_call(model, crit, _ragged([2, 3, 1, 4, 2, 3, 1, 2, 5, 1, 2, 3][: 8 + i % 4], 400 + i), name)
    assert auto.eval_replays >= 1
    r2, l2, g2 = train_step()
    assert r2 and auto.captures == 1 and auto.replays == 3
    assert abs(l1 - l2) <= 1e-6 * max(1.0, abs(l1))
    assert float((g1 - g2).norm()) <= 1e-5 * max(float(g1.norm()), 1e-6)


def test_eval_calls_stay_eager_without_the_opt_in():
    from mesm_amd import synthetic
    args, model, crit = _build()
    name = args.dataset_name
    b = synthetic.to_device(synthetic.workload_batch("C3a", seed=41), DEV)
    for _ in range(3):
        out, _ = _eval_call(model, crit, b, name)
        assert out._eval_losses is None
    auto = model._auto
    assert (auto.eval_captures, auto.eval_replays, auto.eval_eager) == (0, 0, 0)


# ----------------------------------------------------------------------------- end to end
def test_compute_mr_results_with_the_opt_in_equals_without(deterministic_forward):
    from mesm_amd.postprocess import compute_mr_results
    stream = [_ragged(g, 600 + i, ids=100 * i) for i, g in enumerate([[1] * 12, [1] * 12, [1] * 12, [2, 1, 3] * 4])]
    opt = argparse.Namespace(dataset_name="qvhighlights", clip_len=2, max_ts_val=150, sort_results=True)
    res = []
    for on in (True, False):
        args, model, crit = _build(eval=on)
        _seeded(31)
        res.append(compute_mr_results(model, stream, opt, criterion=crit))
        if on:
            assert model._auto.eval_replays >= 2
    (rows_r, meters_r), (rows_e, meters_e) = res
    assert len(rows_r) == len(rows_e) == 12 * 3 + 24
    for a, b in zip(rows_r, rows_e):
        assert (a["qid"], a["query"], a["vid"]) == (b["qid"], b["query"], b["vid"])
        assert a["pred_relevant_windows"] == b["pred_relevant_windows"]
        assert len(a["pred_saliency_scores"]) == len(b["pred_saliency_scores"])
        assert max(abs(x - y) for x, y in zip(a["pred_saliency_scores"], b["pred_saliency_scores"])) <= 1e-2
    assert set(meters_r) == set(meters_e)
    for k in meters_e:
        assert abs(meters_r[k] - meters_e[k]) < 1e-4 * max(1.0, abs(meters_e[k])), k


def test_compute_mr_results_takes_plain_number_loss_entries():
    """a criterion whose loss dict holds plain numbers beside tensors: the meters equal the per-entry float() sums"""
    from io_cases import MR_CASES, StubModel, mr_inputs
    from mesm_amd.postprocess import compute_mr_results

    class Crit(torch.nn.Module):
        weight_dict = {"loss_span": 10.0}

        def forward(self, outputs, batch, is_training=False):
            ls = outputs["pred_spans"].mean()
            return {"loss_span": ls, "count": 0.1, "loss_giou": ls.double() * 3}, 10 * ls

    c = MR_CASES["qvh"]
    loader, outs = mr_inputs(c)
    loader = [{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in b.items()} for b in loader]
    outs = [{k: v.to(DEV) for k, v in o.items()} for o in outs]
    opt = argparse.Namespace(dataset_name="qvh", clip_len=c["clip_len"], max_ts_val=150, sort_results=True)
    _, meters = compute_mr_results(StubModel(outs), loader, opt, criterion=Crit())
    want = {}
    for o in outs:
        ls = o["pred_spans"].mean()
        for k, v in {"loss_span": float(ls) * 10.0, "count": 0.1, "loss_giou": float(ls.double() * 3),
                     "loss_overall": float(10 * ls)}.items():
            want.setdefault(k, []).append(v)
    assert meters == {k: sum(v) / len(v) for k, v in want.items()}
