"""The text cache in the model (MESM.text_cache, mesm_amd/textcache.py): with the switch on, the text stage is a host lookup
of the token-id rows, the frozen CLIP tower on the rows that miss, and the pooling over cache slots -- and every result is
the cache-off model's.  Eager calls compare BITS (outputs, loss entries); the graph paths compare at the suite's
replay-against-eager bounds (1e-4 with the forward deterministic, gradients 1e-4 of their norm).  The model is the
`qvh_clip_tiny` fixture's (tests/test_text_encoder_gpu.py::_build_clip_model's recipe), 6 pairs in groups of 3, 1, 2."""
import argparse
import os

import numpy as np
import pytest
import torch

from golden_io import Fixture

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAME = "qvhighlights"
WORD_KEYS = ("words_id", "words_mask", "words_weight", "unknown_mask", "words_label")


def _build_clip_model(args, sd):
    """build_model reads the text tower's sizes from the checkpoint file: the fixture's `text_encoder.*` tensors go to
    a temporary .pth like the released CLIP weights"""
    import tempfile
    from mesm_amd import build_model
    te = {k[len("text_encoder."):]: v for k, v in sd.items() if k.startswith("text_encoder.")}
    path = os.path.join(tempfile.mkdtemp(), "clip.pth")
    torch.save(te, path)
    args.text_model_path = path
    model = build_model(args)
    model.load_state_dict(sd)
    return model


_FX = []


def fixture():
    if not _FX:
        _FX.append(Fixture("qvh_clip_tiny"))
    return _FX[0]


def make(capacity=None, train=False, **ns):
    """(model, criterion) on the fixture's weights; capacity None: the cache-off twin"""
    from mesm_amd import build_criterion
    fx = fixture()
    args = argparse.Namespace(**fx.cfg)
    args.device = "cuda:0"
    for k, v in ns.items():
        setattr(args, k, v)
    model = _build_clip_model(args, fx.sd)
    crit = build_criterion(args)
    model.train(train)
    crit.train(train)
    if capacity is not None:
        model.text_cache(capacity)
    return model, crit


def variant(order, fresh=()):
    """the fixture's host batch with the word side of pair i taken from pair order[i]; fresh = {pair: tag}: that pair's
    first token id replaced (1 + tag: another query; equal tags on equal sources give equal queries)"""
    b = dict(fixture().batch)
    idx = torch.tensor(order)
    for k in WORD_KEYS:
        b[k] = b[k][idx].clone()
    for i, tag in dict(fresh).items():
        b["words_id"][i, 0] = 1 + tag
    assert int(b["words_id"].max()) < 200
    return b


def to_dev(b):
    from mesm_amd import synthetic
    return synthetic.to_device(b, DEV)


def tensors(tree, prefix=""):
    out = {}
    for k, v in (tree.items() if isinstance(tree, dict) else enumerate(tree)):
        name = "%s%s" % (prefix, k)
        if torch.is_tensor(v):
            out[name] = v
        elif isinstance(v, (dict, list, tuple)):
            out.update(tensors(v, name + "."))
    return out


def bits(t):
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    return t


def step(model, crit, batch, neg=None, mw=None, host=None):
    """one eager training-form step with the given draws -> (outputs {name: tensor}, losses {name: tensor}, total, flat grad)"""
    fx = fixture()
    kw = dict(neg_index=torch.as_tensor(fx.neg_index if neg is None else neg),
              masked_words=torch.as_tensor(fx.masked_words if mw is None else mw))
    if host is not None:
        kw["_host"] = host
    out = model(**batch, dataset_name=NAME, is_training=True, **kw)
    losses, total = crit(out, batch, True)
    model.zero_grad(set_to_none=True)
    total.backward()
    torch.cuda.synchronize()
    return ({k: v.detach().clone() for k, v in tensors(out).items()}, {k: float(v) for k, v in losses.items()},
            total.detach().clone(), model.gradbuf().flat.clone(), out)


def same_bits(got, want):
    (out_a, ls_a, tot_a, flat_a, _), (out_b, ls_b, tot_b, flat_b, _) = got, want
    assert set(out_a) == set(out_b) and len(out_a) > 8
    for k, b in out_b.items():
        a = out_a[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert torch.equal(bits(a), bits(b)), k
    assert ls_a == ls_b and all(np.isfinite(v) for v in ls_b.values())  # (floats: equal values are equal bits)
    assert torch.equal(bits(tot_a), bits(tot_b))
    # (the bound between two eager runs of one batch under this fixture: the backward's atomic sums are not ordered)
    assert float((flat_a - flat_b).norm()) / max(float(flat_b.norm()), 1e-6) < 1e-4


def grad_close(flat_g, flat_e):
    assert float((flat_e - flat_g).norm()) / max(float(flat_e.norm()), 1e-6) < 1e-4


# ----------------------------------------------------------------------------- eager
def test_first_visit_misses_second_visit_hits_and_both_are_the_uncached_step(deterministic_forward):
    from mesm_amd import kernels as kn
    fx = fixture()
    ref, crit_r = make()
    model, crit = make(16)
    assert ref.text_cache_stats() is None
    assert not any(k.startswith("_text") or "cache" in k for k in model.state_dict())
    assert set(model.state_dict()) == set(ref.state_dict())
    batch = to_dev(fx.batch)
    want = step(ref, crit_r, batch)
    towers = []
    orig = kn.clip_embed
    kn.clip_embed = lambda ids, *a: (towers.append(ids.shape[0]), orig(ids, *a))[1]
    try:
        first = step(model, crit, batch)
        s1 = model.text_cache_stats()
        second = step(model, crit, batch)
        s2 = model.text_cache_stats()
    finally:
        kn.clip_embed = orig
    same_bits(first, want)
    same_bits(second, want)
    assert (s1["hits"], s1["misses"], s1["encoded_rows"], s1["entries"], s1["evictions"]) == (0, 6, 6, 6, 0)
    assert (s2["hits"], s2["misses"], s2["encoded_rows"], s2["entries"]) == (6, 6, 6, 6)
    assert towers == [6]  # one tower call over the misses, none on the second visit
    # the fixture comparison of test_training_step_with_clip_tokenizer_matches_reference_golden, at its bounds, cache on
    out = second[4]
    assert out["recfw_words_logit"].shape[-1] == fx.cfg["vocab_size"] + 3

    def errs(a, b):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        return float((a - b).norm() / b.norm().clamp_min(1e-9)), float((a - b).abs().max() / b.abs().max().clamp_min(1e-9))
    for k in ("pred_logits", "pred_spans", "saliency_scores", "neg_saliency_scores", "recfw_words_logit",
              "recon_feat", "projed_words_feat", "expanded_words_feat", "enhanced_video_feat"):
        l2, mx = errs(out[k], fx.out[k])
        assert l2 < 2e-3 and mx < 5e-3, (k, l2, mx)
    assert torch.equal(out["words_mask"].cpu(), fx.out["words_mask"].bool())
    for k, v in fx.losses.items():
        got = float(second[2]) if k == "total" else float(second[1][k])
        assert abs(got - v) < 2e-3 * max(1.0, abs(v)), (k, got, v)
    mq = crit.last_match[0].cpu().tolist()
    got, k = set(), 0
    for b, s in enumerate(fx.match["main.sizes"].tolist()):
        for t_ in range(s):
            got.add((b, mq[k], t_))
            k += 1
    assert got == fx.matched_pairs("main")
    grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert set(grads) == set(fx.grads)

    def l2(a, b):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        return float((a - b).norm()) / max(float(b.norm()), 1e-3 * b.numel() ** 0.5)
    worst = max((l2(grads[n], g), n) for n, g in fx.grads.items())
    assert worst[0] < 5e-2, worst


def test_partial_hits_encode_the_distinct_new_queries_only(deterministic_forward):
    fx = fixture()
    ref, crit_r = make()
    model, crit = make(16)
    step(model, crit, to_dev(fx.batch))
    before = model.text_cache_stats()
    # earlier queries in another order, two new ones, one of them twice
    hb = variant([2, 0, 3, 4, 3, 5], fresh={2: 7, 3: 9, 4: 7})
    assert torch.equal(hb["words_id"][2], hb["words_id"][4]) and not torch.equal(hb["words_id"][2], hb["words_id"][3])
    batch = to_dev(hb)
    # the host copy of the ids rides along like the collate's `_host` does: no fetch
    got = step(model, crit, batch, host={"words_id": hb["words_id"]})
    same_bits(got, step(ref, crit_r, batch))
    after = model.text_cache_stats()
    assert after["encoded_rows"] - before["encoded_rows"] == 2
    assert after["hits"] - before["hits"] == 3 and after["misses"] - before["misses"] == 3
    assert after["entries"] == 8
    # and without the host copy (a small fetch): all hits now
    same_bits(step(model, crit, batch), got)
    assert model.text_cache_stats()["encoded_rows"] == after["encoded_rows"]


def test_eviction_keeps_results_equal_to_the_uncached_model(deterministic_forward):
    ref, crit_r = make()
    model, crit = make(7)  # the batch's distinct queries + 1
    batches = [variant(range(6)), variant(range(6), fresh={i: 20 + i for i in range(6)}),
               variant([5, 4, 3, 2, 1, 0], fresh={i: 40 + i for i in range(5)})]
    for hb in batches + batches[:1]:
        b = to_dev(hb)
        same_bits(step(model, crit, b), step(ref, crit_r, b))
    s = model.text_cache_stats()
    assert s["evictions"] > 0 and s["entries"] == 7 and s["capacity"] == 7
    # a batch with more distinct queries than slots is refused before anything changes
    small, crit_s = make(5)
    with pytest.raises(ValueError, match="6 distinct.*capacity 5"):
        step(small, crit_s, to_dev(batches[0]))
    assert small.text_cache_stats()["entries"] == 0 and small.text_cache_stats()["misses"] == 0


def test_new_tower_weights_invalidate_the_cache(deterministic_forward):
    from mesm_amd import checkpoint
    fx = fixture()
    ref, crit_r = make()
    model, crit = make(16)
    batch = to_dev(fx.batch)
    stale = step(model, crit, batch)
    te = {k: v.clone() for k, v in model.text_encoder.state_dict().items()}
    te["ln_final.weight"] = te["ln_final.weight"] * 1.5
    te["ln_final.bias"] = te["ln_final.bias"] + 0.25
    model.text_encoder.load_state_dict(te)
    ref.text_encoder.load_state_dict(te)
    s = model.text_cache_stats()
    assert s["entries"] == 0 and s["generation"] == 1 and s["evictions"] == 0
    got = step(model, crit, batch)
    same_bits(got, step(ref, crit_r, batch))
    assert not torch.equal(got[0]["projed_words_feat"], stale[0]["projed_words_feat"])
    assert model.text_cache_stats()["encoded_rows"] == 12
    # the same through the model's own load_state_dict
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd["text_encoder.ln_final.bias"] = sd["text_encoder.ln_final.bias"] - 0.5
    model.load_state_dict(sd)
    ref.load_state_dict(sd)
    assert model.text_cache_stats()["entries"] == 0
    got2 = step(model, crit, batch)
    same_bits(got2, step(ref, crit_r, batch))
    assert not torch.equal(got2[0]["projed_words_feat"], got[0]["projed_words_feat"])
    # a checkpoint resume (the tower's weights merged back, checkpoint.load_checkpoint) leaves a valid, empty cache
    ckpt = {"model": checkpoint.state_dict_without_module(model, "text_encoder"), "epoch": 3}
    assert checkpoint.load_checkpoint(ckpt, model, resume_all=True) == 4
    assert model.text_cache_stats()["entries"] == 0
    same_bits(step(model, crit, batch), got2)
    # clear() by hand, and .half() / .float() round trips of the module tree
    model._active_text_cache().clear()
    assert model.text_cache_stats()["entries"] == 0
    gen = model.text_encoder.weights_generation
    model.text_encoder.float()
    assert model.text_encoder.weights_generation > gen
    from mesm_amd.text_encoder import convert_weights
    gen = model.text_encoder.weights_generation
    convert_weights(model.text_encoder)
    assert model.text_encoder.weights_generation > gen


def test_refusals_and_switches(monkeypatch):
    import tempfile
    from mesm_amd import build_model, synthetic
    # no encoder (pre-extracted word features)
    plain = build_model(synthetic.make_args("C3b", device="cuda:0"))
    with pytest.raises(ValueError, match="no text encoder"):
        plain.text_cache(8)
    # a GloVe-built model
    path = os.path.join(tempfile.mkdtemp(), "glove.txt")
    with open(path, "w") as f:
        for w in ("a", "b", "<PAD>"):
            f.write(w + " " + " ".join("0.5" for _ in range(300)) + "\n")

    class Vocab:
        wtoi = {"<PAD>": 0, "a": 1, "b": 2}

        def __len__(self):
            return 3
    gargs = synthetic.make_args("C1", device="cuda:0", tokenizer_type="GloVeSimple", text_model_path=path)
    glove = build_model(gargs, Vocab())
    with pytest.raises(ValueError, match="GloVe"):
        glove.text_cache(8)
    gargs.text_cache = 8
    with pytest.raises(ValueError, match="GloVe"):
        build_model(gargs, Vocab())
    # build_model with the option in the namespace; the environment for a loop that is not to be edited
    model, _ = make(text_cache=12)
    assert model.text_cache_stats()["capacity"] == 12
    with pytest.raises(ValueError, match="at least 1"):
        model.text_cache(0)
    off, _ = make()
    assert off.text_cache_stats() is None
    monkeypatch.setenv("MESM_TEXT_CACHE", "9")
    assert off.text_cache_stats()["capacity"] == 9
    assert model.text_cache_stats()["capacity"] == 12  # (an explicit call wins)
    off.text_cache(None)
    assert off.text_cache_stats() is None
    with pytest.raises(ValueError, match="MESM_TEXT_CACHE"):
        plain.text_cache_stats()
    monkeypatch.delenv("MESM_TEXT_CACHE")
    assert plain.text_cache_stats() is None


# ----------------------------------------------------------------------------- graph paths
def _eager_ref(ref, crit_r, hb, draws):
    neg, mw = draws  # (of a pair-padded step: the real pairs' entries)
    return step(ref, crit_r, to_dev(hb), neg=neg[:6], mw=mw[:6])


def _loss_close(got, want, what):
    assert abs(float(got) - float(want)) < 1e-4 * max(1.0, abs(float(want))), (what, float(got), float(want))


@pytest.mark.parametrize("pairs", [None, 8])
def test_step_cache_replays_other_queries_from_one_graph(pairs, deterministic_forward):
    from mesm_amd.graphed import StepCache
    ref, crit_r = make()
    model, crit = make(16)
    cache = StepCache(model, crit, NAME, pairs=pairs)
    b0 = variant(range(6))
    _, gs = cache.run(b0)
    torch.cuda.synchronize()
    assert gs._tc is model._active_text_cache() and hasattr(gs.plan, "text_slots")
    assert gs.plan.text_slots.dtype == torch.int32 and gs.plan.text_slots.shape == (8 if pairs else 6,)
    s0 = model.text_cache_stats()
    assert s0["encoded_rows"] == 6  # the capture's warm-up passes count nothing
    # same bucket, other queries: three cached (re-ordered), two new, one of them twice... and one kept
    b1 = variant([2, 0, 3, 4, 3, 5], fresh={2: 7, 3: 9, 4: 7})
    for k, hb in enumerate((b0, b1, b1)):
        total_g, gs2 = cache.run(hb)
        torch.cuda.synchronize()
        assert gs2 is gs and cache.captures == 1
        flat_g = model.gradbuf().flat.clone()
        _, ls_e, tot_e, flat_e, _ = _eager_ref(ref, crit_r, hb, gs._draws)
        _loss_close(total_g, tot_e, "total")
        for name, v in gs.losses.items():
            _loss_close(v, ls_e[name], name)
        grad_close(flat_g, flat_e)
        s = model.text_cache_stats()
        assert s["encoded_rows"] == (6, 8, 8)[k]  # an all-hit replay encodes nothing
    if pairs:
        # padding pairs are copies of pair 0 and take its slot
        sl = gs.plan.text_slots.cpu()
        assert int(sl[6]) == int(sl[7]) == int(sl[0])
    # flipping the switch never replays a graph captured under the other setting
    model.text_cache(None)
    with pytest.raises(ValueError, match="text cache"):
        gs.load_batch(b1)
    with pytest.raises(RuntimeError, match="text cache"):
        gs.run()
    total_off, gs_off = cache.run(b1)
    torch.cuda.synchronize()
    assert gs_off is not gs and cache.captures == 2 and gs_off._tc is None and not hasattr(gs_off.plan, "text_slots")
    _, _, tot_e, flat_e, _ = _eager_ref(ref, crit_r, b1, gs_off._draws)
    _loss_close(total_off, tot_e, "total, cache off")
    model.text_cache(16)
    with pytest.raises(ValueError, match="text cache"):
        gs_off.load_batch(b1)
    total_on, gs_on = cache.run(b1)
    torch.cuda.synchronize()
    assert gs_on is not gs_off and gs_on is not gs  # (a new cache buffer: the old graph reads the old one)
    _, _, tot_e, _, _ = _eager_ref(ref, crit_r, b1, gs_on._draws)
    _loss_close(total_on, tot_e, "total, cache on again")


def test_new_tower_weights_reach_a_loaded_graph(deterministic_forward):
    from mesm_amd.graphed import StepCache
    ref, crit_r = make()
    model, crit = make(16)
    cache = StepCache(model, crit, NAME)
    b0 = variant(range(6))
    cache.run(b0)
    total_a, gs = cache.run(b0)
    total_a = float(total_a)
    te = {k: v.clone() for k, v in model.text_encoder.state_dict().items()}
    te["ln_final.weight"] = te["ln_final.weight"] * 1.5
    model.text_encoder.load_state_dict(te)
    ref.text_encoder.load_state_dict(te)
    total_b = float(gs.run(redraw=False))  # no load_batch in between: the step looks its batch up again
    _, _, tot_e, _, _ = _eager_ref(ref, crit_r, b0, gs._draws)
    _loss_close(total_b, tot_e, "total after load_state_dict")
    assert total_b != total_a and cache.captures == 1


def test_autograph_replays_with_the_cache_on(deterministic_forward):
    ref, crit_r = make()
    model, crit = make(16)
    model.autograph(True)
    auto = model._auto
    hbs = [variant(range(6)), variant([1, 2, 3, 4, 5, 0]), variant([2, 0, 3, 4, 3, 5], fresh={2: 7, 3: 9, 4: 7}),
           variant([2, 0, 3, 4, 3, 5], fresh={2: 7, 3: 9, 4: 7})]
    encoded, steps = [], []
    for i, hb in enumerate(hbs):
        batch = to_dev(hb)
        out = model(**batch, dataset_name=NAME, is_training=True)
        losses, total = crit(out, batch, True)
        model.zero_grad(set_to_none=True)
        total.backward()
        torch.cuda.synchronize()
        encoded.append(model.text_cache_stats()["encoded_rows"])
        st = out._auto_step
        steps.append(st)
        if st is None:
            continue
        flat_g = model.gradbuf().flat.clone()
        out_g = {k: v.detach().clone() for k, v in tensors(out).items()}
        out_e, ls_e, tot_e, flat_e, _ = _eager_ref(ref, crit_r, hb, st._draws)
        _loss_close(total.detach(), tot_e, "total")
        for k, v in losses.items():
            _loss_close(v, ls_e[k], k)
        assert set(out_g) == set(out_e)
        for k, v in out_g.items():
            if v.dtype.is_floating_point:
                d = float((out_e[k].double() - v.double()).abs().max())
                assert d <= 1e-4 * max(1.0, float(out_e[k].double().abs().max())), (k, d)
            else:
                assert torch.equal(out_e[k], v), k
        grad_close(flat_g, flat_e)
    assert [s is not None for s in steps] == [False, True, True, True]
    assert steps[1] is steps[2] is steps[3] and (auto.eager, auto.captures, auto.replays) == (1, 1, 3)
    assert encoded == [6, 6, 8, 8]  # no new capture when only slots change; an all-hit replay encodes nothing
    # the switch flips: the captured graph is not replayed, the bucket gets another one
    model.text_cache(None)
    batch = to_dev(hbs[1])
    out = model(**batch, dataset_name=NAME, is_training=True)
    losses, total = crit(out, batch, True)
    model.zero_grad(set_to_none=True)
    total.backward()
    torch.cuda.synchronize()
    assert out._auto_step is not None and out._auto_step is not steps[1] and auto.captures == 2
    assert out._auto_step._tc is None
    _, _, tot_e, flat_e, _ = _eager_ref(ref, crit_r, hbs[1], out._auto_step._draws)
    _loss_close(total.detach(), tot_e, "total, cache off")


def test_eval_graph_replays_with_the_cache_on(deterministic_forward):
    from test_eval_graph_gpu import _compare, _compare_losses, _eval_call, _seeded
    ref, crit_r = make()
    model, crit = make(16)
    model.autograph(True, eval=True)
    auto = model._auto
    hbs = [variant(range(6)), variant([1, 2, 3, 4, 5, 0]), variant([2, 0, 3, 4, 3, 5], fresh={2: 7, 3: 9, 4: 7}),
           variant([2, 0, 3, 4, 3, 5], fresh={2: 7, 3: 9, 4: 7})]
    encoded = []
    for i, hb in enumerate(hbs):
        b = to_dev(hb)
        _seeded(300 + i)
        out_r, res_r = _eval_call(model, crit, b, NAME)
        encoded.append(model.text_cache_stats()["encoded_rows"])
        _seeded(300 + i)
        out_e, res_e = _eval_call(ref, crit_r, b, NAME)
        _compare(out_r, out_e)
        _compare_losses(res_r, res_e)
    assert (auto.eval_eager, auto.eval_captures, auto.eval_replays) == (1, 1, 3)
    assert encoded == [6, 6, 8, 8]
    model.text_cache(None)
    _seeded(400)
    out_r, res_r = _eval_call(model, crit, to_dev(hbs[2]), NAME)
    _seeded(400)
    out_e, res_e = _eval_call(ref, crit_r, to_dev(hbs[2]), NAME)
    _compare(out_r, out_e)
    assert auto.eval_captures == 2  # the graph captured with the cache on was not replayed


def test_a_batch_prepared_by_the_loader_pipeline_gets_its_slots_in_the_training_process(deterministic_forward):
    """loader.HostPipeline (what loader workers run) knows no model: its arrays carry no slots; StepCache.run_prepared
    looks the queries up where the table lives, encodes the misses and replays the bucket's graph"""
    from mesm_amd.graphed import StepCache
    ref, crit_r = make()
    model, crit = make(16)
    cache = StepCache(model, crit, NAME, pairs=8)
    b0, b1 = variant(range(6)), variant([2, 0, 3, 4, 3, 5], fresh={2: 7, 3: 9, 4: 7})
    _, gs = cache.run(b0)
    prep = cache.pipeline().prepare(b1)
    assert "p.text_slots" not in prep["arr"]
    total_g, gs2 = cache.run_prepared(prep)
    torch.cuda.synchronize()
    assert gs2 is gs and cache.captures == 1
    flat_g = model.gradbuf().flat.clone()
    _, _, tot_e, flat_e, _ = _eager_ref(ref, crit_r, b1, gs._draws)
    _loss_close(total_g, tot_e, "total")
    grad_close(flat_g, flat_e)
    assert model.text_cache_stats()["encoded_rows"] == 8
    sl = gs.plan.text_slots.cpu()
    assert int(sl[2]) == int(sl[4]) and int(sl[6]) == int(sl[7]) == int(sl[0])
