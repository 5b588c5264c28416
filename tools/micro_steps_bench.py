"""Micro-batched graph replays next to today's loop at C3a (32 pairs, train mode): ms per replay, host clock around
REPLAYS replays with one synchronisation at the end (the host work of FlatAdamW.step() is part of what is compared).

One process alternates four forms, each on its own copy of the model (the micro-stepped graphs of one model share its
cycle state):

  (a) a plain GraphedStep, then the host call opt.step(grad_clip=0.1) after every replay -- the baseline;
  (b) micro_steps=1, optimizer=opt: the same update, captured in the graph;
  (c) micro_steps=8, optimizer=opt: one captured update per 8 replays;
  (d) micro_steps=8 without an optimizer: accumulation alone, no update at all.

(c) and (d) do less work per replay than (a) by construction (7 of 8 clears and updates fall away); (b) against (a) is
the like-for-like comparison.  The yardstick is (a)'s own round-to-round spread in the same run.

Usage: python tools/micro_steps_bench.py [--rounds 7] [--replays 40]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mesm_amd import build_criterion, build_model, synthetic
from mesm_amd.graphed import GraphedStep
from mesm_amd.optim import FlatAdamW

CLIP = 0.1


def make(form):
    args = synthetic.make_args("C3a", device="cuda:0")
    torch.manual_seed(0)
    model = build_model(args)
    crit = build_criterion(args)
    model.train()
    opt = FlatAdamW(model, lr=1e-4, weight_decay=1e-2)
    batch = synthetic.to_device(synthetic.workload_batch("C3a", seed=1), torch.device("cuda:0"))
    kw = {"a": {}, "b": dict(micro_steps=1, optimizer=opt, grad_clip=CLIP),
          "c": dict(micro_steps=8, optimizer=opt, grad_clip=CLIP), "d": dict(micro_steps=8)}[form]
    g = GraphedStep(model, crit, batch, args.dataset_name, warmup=2, **kw)
    if form == "a":
        def replay():
            g.run()
            opt.step(grad_clip=CLIP)
    else:
        replay = g.run
    return replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replays", type=int, default=40)
    a = ap.parse_args()
    if a.replays % 8:
        ap.error("--replays must be a multiple of 8 (whole cycles)")
    names = {"a": "plain graph + host opt.step", "b": "micro_steps=1, optimizer captured",
             "c": "micro_steps=8, optimizer captured", "d": "micro_steps=8, no optimizer"}
    forms = {f: make(f) for f in names}
    for fn in forms.values():  # warm-up: code objects, clocks, whole cycles
        for _ in range(16):
            fn()
    torch.cuda.synchronize()
    ms = {f: [] for f in forms}
    for _ in range(a.rounds):
        for f, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.replays):
                fn()
            torch.cuda.synchronize()
            ms[f].append(1e3 * (time.perf_counter() - t0) / a.replays)
    res = {"workload": "C3a", "rounds": a.rounds, "replays_per_round": a.replays, "forms": {}}
    print("C3a, train mode, %d rounds x %d replays per form" % (a.rounds, a.replays))
    for f, t in ms.items():
        med = statistics.median(t)
        res["forms"][f] = {"name": names[f], "ms_per_replay_median": med, "ms_per_replay_min": min(t),
                           "ms_per_replay_max": max(t), "spread_rel": (max(t) - min(t)) / med, "ms_per_replay_rounds": t}
        print("(%s) %-36s %.4f ms/replay (min %.4f, max %.4f, spread %.2f%%)"
              % (f, names[f], med, min(t), max(t), 100 * (max(t) - min(t)) / med))
    base = res["forms"]["a"]
    for f in ("b", "c", "d"):
        d = res["forms"][f]["ms_per_replay_median"] / base["ms_per_replay_median"] - 1
        res["forms"][f]["vs_a_rel"] = d
        print("(%s) against (a): %+.2f%% ((a)'s own spread: %.2f%%)" % (f, 100 * d, 100 * base["spread_rel"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
