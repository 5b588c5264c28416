"""The frozen CLIP text tower and the text cache (mesm_amd/textcache.py, MESM.text_cache), timed on the flagship shapes.

One process, the forms alternating round by round, every form timed with device events around STEPS calls that end in a
synchronise:

  (a) the tower alone on 32 x 77 token ids at the released size (width 512, 8 heads, 12 layers, vocabulary 49408)
  (b) an eager C3a training step from token ids (synthetic.with_clip_tokens), cache off
  (c) the same step with every query cached (all hits)
  (d) the same step with every query a miss (the table emptied before every step: lookup + tower + store + pooling)
  (e) the step replayed through graphed.StepCache, cache off against all-hit, with the dispatch count of each graph
      (kernel launches recorded by torch.profiler over one replay)

The yardstick is (b) (eager) and the cache-off replay (graph) of the same run, each with its round-to-round spread.  The
weights are random (the released CLIP weights are not part of the repository); times do not depend on their values.

Usage: python tools/text_cache_bench.py [--rounds 5] [--steps 20]"""
import argparse
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MESM_AUTOGRAPH", "0")  # (b)-(d) are eager steps; (e) replays through StepCache explicitly
import torch

from mesm_amd import build_criterion, build_model, synthetic
from mesm_amd.graphed import StepCache
from mesm_amd.text_encoder import CLIPTextEncoder

DEV = torch.device("cuda:0")
VOCAB = 49408


def build(cache):
    """the C3a model with the released text tower's sizes (random weights), train mode; cache: capacity or None"""
    torch.manual_seed(0)
    enc = CLIPTextEncoder(512, 77, VOCAB, 512, 8, 12)
    path = os.path.join(tempfile.mkdtemp(), "clip_text_encoder.pth")
    torch.save(enc.state_dict(), path)
    args = synthetic.make_args("C3a", device="cuda:0", tokenizer_type="CLIP", load_vocab_pkl=False, text_model_path=path,
                               vocab_size=5000)
    torch.manual_seed(1)
    model = build_model(args)
    crit = build_criterion(args)
    model.train()
    crit.train()
    if cache is not None:
        model.text_cache(cache)
    return args, model, crit


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def dispatches(fn):
    """kernel launches of one call of fn (a graph replay: the kernels of its nodes)"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and not e.name.lower().startswith(("memcpy", "memset")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-dispatch-count", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/text_cache_bench.py measures on an MI355X: no device found")
    name = "qvhighlights"
    host = synthetic.with_clip_tokens(synthetic.workload_batch("C3a", seed=0), vocab=VOCAB)
    batch = synthetic.to_device(host, DEV)
    batch["_host"] = {"words_id": host["words_id"]}  # what the collate keeps (batching.attach_host_side): no fetch
    N = host["words_id"].shape[0]
    _, m_off, c_off = build(None)
    _, m_on, c_on = build(4 * N)
    # the replayed forms get models of their own, never stepped eagerly: autograd pins a parameter's AccumulateGrad node to
    # the stream of its first backward, and a model whose first backward ran on the default stream (MESM_AUTOGRAPH=0 above)
    # cannot be captured on the capture stream afterwards (graphed.capture_stream)
    _, g_off, gc_off = build(None)
    _, g_on, gc_on = build(4 * N)

    def eager(model, crit):
        def fn():
            out = model(**batch, dataset_name=name, is_training=True)
            _, total = crit(out, batch, True)
            model.zero_grad(set_to_none=True)
            total.backward()
        return fn

    def all_miss():
        m_on._active_text_cache().clear()
        eager(m_on, c_on)()

    ids = batch["words_id"]
    forms = [("(a) tower alone, 32 x 77", lambda: m_off.text_encoder(ids)),
             ("(b) eager step, cache off", eager(m_off, c_off)),
             ("(c) eager step, all hits", eager(m_on, c_on)),
             ("(d) eager step, all misses", all_miss)]
    # (e): one StepCache per model; host batches like a loader's
    sc_off, sc_on = StepCache(g_off, gc_off, name), StepCache(g_on, gc_on, name)
    forms += [("(e) replayed step, cache off", lambda: sc_off.run(host)),
              ("(e) replayed step, all hits", lambda: sc_on.run(host))]
    for _, fn in forms:  # warm-up: code objects, captures, the cache's first fill
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {n_: [] for n_, _ in forms}
    for _ in range(a.rounds):
        for n_, fn in forms:
            ms[n_].append(timed(fn, a.steps))
    res = {"pairs": N, "rounds": a.rounds, "steps_per_round": a.steps, "forms": {}, "cache_eager": m_on.text_cache_stats(),
           "cache_replayed": g_on.text_cache_stats()}
    print("%d pairs, %d rounds x %d calls per form" % (N, a.rounds, a.steps))
    for n_, _ in forms:
        t = ms[n_]
        med = statistics.median(t)
        res["forms"][n_] = {"ms_median": med, "ms_min": min(t), "ms_max": max(t), "spread_rel": (max(t) - min(t)) / med,
                            "ms_rounds": t}
        print("%-30s %.3f ms (min %.3f, max %.3f, spread %.1f%%)" % (n_, med, min(t), max(t), 100 * (max(t) - min(t)) / med))
    f = res["forms"]
    for base, others in (("(b) eager step, cache off", ("(c) eager step, all hits", "(d) eager step, all misses")),
                         ("(e) replayed step, cache off", ("(e) replayed step, all hits",))):
        for o in others:
            d = f[o]["ms_median"] - f[base]["ms_median"]
            f[o]["vs_cache_off_ms"] = d
            print("%s against %s: %+.3f ms (%+.1f%%; the spread of the cache-off form: %.1f%%)"
                  % (o, base, d, 100 * d / f[base]["ms_median"], 100 * f[base]["spread_rel"]))
    if not a.no_dispatch_count:
        gs_off, gs_on = sc_off.run(host)[1], sc_on.run(host)[1]
        try:
            res["dispatches"] = {"replay, cache off": dispatches(lambda: gs_off.graph.replay()),
                                 "replay, all hits": dispatches(lambda: gs_on.graph.replay()),
                                 "tower alone": dispatches(lambda: m_off.text_encoder(ids))}
        except Exception as e:  # (a profiler that does not see graph kernels: said, not guessed)
            res["dispatches"] = "not measured (%s: %s)" % (type(e).__name__, e)
        print("dispatches per call:", res["dispatches"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
