"""Evaluation loop timing on one MI355X: the reference's eval.py:52-117 per-batch work (forward with is_training=False
under no_grad, criterion with is_training=False, submission rows, saliency rows, loss meters) over a loader-shaped
stream -- 36 batches of 12 video groups at C3a shapes, group sizes drawn like bench.py's loader-like section -- in
three forms:

  eager          model.autograph(eval=False); rows / saliency / meters by the host path (predict_windows, saliency_rows,
                 one float() per loss entry: what compute_mr_results did before device rows)
                 (host_postprocess_ms_per_batch: the time after each forward returns, for every form)
  replayed       model.autograph(eval=True, pad=(75, 32), pairs=8); the same host path
  replayed_rows  the same replays; postprocess.compute_mr_results (device rows, one transfer per batch)

Every form runs the stream twice (the first pass captures the graphs of its buckets) and times the second.  Prints one
JSON line.  `--only FORM --passes K` runs one form K times without the report (for a rocprofv3 run of its own).

    python tools/eval_bench.py [--only replayed_rows --passes 2] [--feature-dtype float16]

--feature-dtype float16: the stream's video features are stored as float16 (mesm_amd.FEATURE_DTYPES); the report says so.
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

FORMS = ("eager", "replayed", "replayed_rows")


def stream(wl, nb=36, videos=12, seed=5, feature_dtype=None):
    from mesm_amd import synthetic
    rng = random.Random(seed)
    sizes, probs = list(range(1, 10)), [0.18, 0.22, 0.20, 0.15, 0.10, 0.07, 0.04, 0.025, 0.015]
    out, qid = [], 0
    dev = torch.device("cuda:0")
    for i in range(nb):
        groups = [rng.choices(sizes, probs)[0] for _ in range(videos)]
        b = synthetic.make_batch(wl["dataset_name"], groups, wl["Lv"], wl["Lw"], wl["v_feat_dim"], wl["t_feat_dim"],
                                 wl["vocab_size"] + 1, seed=2000 + i, ragged=True, feature_dtype=feature_dtype)
        b = synthetic.to_device(b, dev)
        n = sum(groups)
        b["qid"] = list(range(qid, qid + n))
        b["sentence"] = ["q%d" % j for j in range(qid, qid + n)]
        b["video_id"] = ["v%d" % j for j in range(qid, qid + n)]
        qid += n
        out.append(b)
    return out


def host_pass(model, crit, batches, opt):
    """eval.py:63-105 with the host post-processing of predict_windows / saliency_rows / float() per loss entry"""
    from mesm_amd.postprocess import predict_windows, saliency_rows
    post = 0.0
    res = []
    for b in batches:
        out = model(**b, dataset_name=opt.dataset_name, is_training=False)
        loss_dict, loss = crit(out, b, is_training=False)
        t = time.perf_counter()
        rows = predict_windows(out["pred_logits"], out["pred_spans"], b["duration"], clip_len=opt.clip_len,
                               max_ts_val=opt.max_ts_val)
        sal = saliency_rows(out["saliency_scores"], b["video_mask"])
        meters = {k: float(v) for k, v in loss_dict.items()}
        meters["loss_overall"] = float(loss)
        post += time.perf_counter() - t
        res.append((rows, sal, meters))
    return post, res


class _Timed:
    """the model as compute_mr_results sees it, noting when each forward returns and the next one starts: the time in
    between is that batch's post-processing (device rows, the one transfer, the row dicts, the loss meters)"""

    def __init__(self, model):
        self.model, self.post, self.back = model, 0.0, None

    def eval(self):
        self.model.eval()
        return self

    def __call__(self, **kw):
        t = time.perf_counter()
        if self.back is not None:
            self.post += t - self.back
        out = self.model(**kw)
        self.back = time.perf_counter()
        return out

    def close(self):
        if self.back is not None:
            self.post += time.perf_counter() - self.back
            self.back = None
        return self.post


def run_form(form, model, crit, batches, opt, passes=2):
    from mesm_amd.postprocess import compute_mr_results
    model.autograph(True, eval=form != "eager", pad=(75, 32), pairs=8)
    times, posts = [], []
    for _ in range(passes):
        torch.cuda.synchronize()
        window = [time.monotonic_ns()]
        t = time.perf_counter()
        with torch.no_grad():
            if form == "replayed_rows":
                timed = _Timed(model)
                compute_mr_results(timed, batches, opt, criterion=crit)
                post = timed.close()
            else:
                post, _ = host_pass(model, crit, batches, opt)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
        window.append(time.monotonic_ns())
        posts.append(post)
    return times, posts, window


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=FORMS)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--batches", type=int, default=36)
    ap.add_argument("--feature-dtype", choices=("float32", "float16"), default="float32")
    a = ap.parse_args()
    from mesm_amd import build_criterion, build_model, synthetic
    wl = synthetic.WORKLOADS["C3a"]
    args = synthetic.make_args("C3a", device="cuda:0")
    torch.manual_seed(0)
    batches = stream(wl, nb=a.batches, feature_dtype=getattr(torch, a.feature_dtype))
    queries = sum(b["video_feat"].shape[0] for b in batches)
    opt = argparse.Namespace(dataset_name=args.dataset_name, clip_len=2, max_ts_val=150, sort_results=True)
    report = {"workload": "C3a", "feature_dtype": a.feature_dtype, "batches": len(batches), "videos_per_batch": 12, "queries": queries,
              "pad": [75, 32], "pairs": 8, "forms": {}}
    for form in ([a.only] if a.only else FORMS):
        torch.manual_seed(1)
        model = build_model(args)
        crit = build_criterion(args)
        model.eval()
        crit.eval()
        model.autograph(True)  # (the caller's criterion introduces itself on the first eager call, as in eval.py)
        times, posts, window = run_form(form, model, crit, batches, opt, passes=a.passes)
        auto = model._auto
        tt = times[-1]
        report["forms"][form] = {
            "ms_per_batch": tt / len(batches) * 1e3, "queries_per_s": queries / tt,
            "first_pass_ms_per_batch": times[0] / len(batches) * 1e3,
            "graphs_captured": auto.eval_captures, "eval_replays": auto.eval_replays, "eval_eager": auto.eval_eager,
            "host_postprocess_ms_per_batch": posts[-1] / len(batches) * 1e3,
            "timed_pass_monotonic_ns": window}  # (CLOCK_MONOTONIC: the window of a kernel trace that is the timed pass)
        del model, crit
        torch.cuda.empty_cache()
    if not a.only:
        f = report["forms"]
        report["speedup_replayed_rows_vs_eager"] = f["eager"]["ms_per_batch"] / f["replayed_rows"]["ms_per_batch"]
        report["note"] = ("second pass over the stream, graphs warm; eager / replayed: host post-processing by "
                          "predict_windows + saliency_rows + float() per loss entry; replayed_rows: postprocess.compute_mr_results with "
                          "device rows, its post-processing = everything between a forward's return and the next forward "
                          "(criterion, device rows, the one transfer, row dicts, meters); every post-processing time is part "
                          "of ms_per_batch and includes waiting for the device")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
