"""The AdamW update with the weight EMA fused in, next to the update without it and to the update plus a separate
whole-buffer lerp_, on the flagship model's flat buffers (C3a: 13.7 M elements).

One process alternates three forms -- (a) mesm_adamw_step, (b) mesm_adamw_step_ema, (c) mesm_adamw_step followed by
`ema.lerp_(p, 1 - d)` -- and times each with device events over LAUNCHES updates per round.  (a) moves 28 B per element,
(b) 36 B, (c) 28 B plus the 12 B of the lerp_ in a second launch; the yardstick is (a) in the same run, with its own
round-to-round spread.

Usage: python tools/ema_bench.py [--rounds 7] [--launches 200]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mesm_amd import _lib, build_model, synthetic
from mesm_amd._lib import check, lib, ptr, stream_ptr

DECAY = 0.999


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = build_model(synthetic.make_args("C3a", device="cuda:0"))
    n = model.gradbuf().numel
    start = model.flat_params()
    g = 1e-3 * torch.randn(n, device=dev)
    step_t = torch.full((1,), 10, device=dev, dtype=torch.int32)
    lr_t = torch.full((1,), 1e-4, device=dev, dtype=torch.float32)
    active = torch.ones(n // 4, device=dev, dtype=torch.uint8)
    es = torch.frombuffer(bytearray(bytes(_lib.EmaState(decay=DECAY, warmup=0, step0=0, reserved=0))),
                          dtype=torch.uint8).to(dev)
    dout = torch.zeros(1, device=dev)

    def state():
        return start.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev), start.clone()

    def head(p, m, v):
        return (ptr(p), ptr(g), ptr(m), ptr(v), ptr(active), n, None, 0, 0.0, ptr(lr_t), 0.9, 0.999, 1e-8, 1e-2, ptr(step_t),
                None)

    def plain(p, m, v, e):
        check(lib().mesm_adamw_step(*head(p, m, v), stream_ptr()), "mesm_adamw_step")

    def fused(p, m, v, e):
        check(lib().mesm_adamw_step_ema(*head(p, m, v), ptr(e), ptr(es), ptr(dout), stream_ptr()), "mesm_adamw_step_ema")

    def separate(p, m, v, e):
        plain(p, m, v, e)
        e.lerp_(p, 1.0 - DECAY)

    # bytes an update moves per element, one active byte per 4 elements on top
    forms = [("(a) update", plain, 28), ("(b) update + fused EMA", fused, 36), ("(c) update, then lerp_", separate, 40)]
    runs = [(name, fn, per * n + n // 4, state()) for name, fn, per in forms]
    for _, fn, _, st in runs:  # warm-up: code objects, clocks
        for _ in range(20):
            fn(*st)
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _, _ in runs}
    for _ in range(a.rounds):
        for name, fn, _, st in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn(*st)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.launches)
    res = {"elements": n, "rounds": a.rounds, "launches_per_round": a.launches, "forms": {}}
    print("%d elements, %d rounds x %d updates per form" % (n, a.rounds, a.launches))
    for name, _, nbytes, _ in runs:
        t = ms[name]
        med = statistics.median(t)
        res["forms"][name] = {"ms_per_update_median": med, "ms_per_update_min": min(t), "ms_per_update_max": max(t),
                              "spread_rel": (max(t) - min(t)) / med, "bytes_per_update": nbytes,
                              "GBps_median": nbytes / med / 1e6, "ms_per_update_rounds": t}
        print("%-26s %.4f ms/update (min %.4f, max %.4f, spread %.2f%%)  %7.0f GB/s  over %.1f MB"
              % (name, med, min(t), max(t), 100 * (max(t) - min(t)) / med, nbytes / med / 1e6, nbytes / 1e6))
    base = res["forms"]["(a) update"]
    for name, _, _, _ in runs[1:]:
        d = res["forms"][name]["ms_per_update_median"] / base["ms_per_update_median"] - 1
        res["forms"][name]["vs_a_rel"] = d
        print("%s against (a): %+.1f%% (the spread of (a) itself: %.2f%%)" % (name, 100 * d, 100 * base["spread_rel"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
