"""mesm_adamw_step_groups next to mesm_adamw_step on the flagship model's flat buffers (C3a: 13.7 M elements).

One process alternates three forms of the same update -- the old entry, the new entry with one group, the new entry
with the four groups of tests/test_optim_groups_gpu.py (decoder at 0.1 x lr, no decay on 1-d tensors, the SS
reconstructor frozen) -- and times each with device events over LAUNCHES launches per round.  All forms move the same
bytes, so the yardstick is the old entry in the same run: its own round-to-round spread.

Usage: python tools/optim_groups_bench.py [--rounds 7] [--launches 200]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mesm_amd import _lib, build_model, synthetic
from mesm_amd._lib import check, lib, ptr, stream_ptr
from mesm_amd.optim import param_groups, tag_table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = build_model(synthetic.make_args("C3a", device="cuda:0"))
    gb = model.gradbuf()
    n = gb.numel
    start = model.flat_params()
    g = 1e-3 * torch.randn(n, device=dev)
    step_t = torch.full((1,), 10, device=dev, dtype=torch.int32)
    lr_t = torch.full((1,), 1e-4, device=dev, dtype=torch.float32)

    def table(rows):
        arr = (_lib.AdamGroup * len(rows))()
        for r, (lr, wd) in zip(arr, rows):
            r.lr, r.beta1, r.beta2, r.eps, r.weight_decay, r.step0 = lr, 0.9, 0.999, 1e-8, wd, 0
        return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)

    groups = param_groups(model, [("transformer.decoder.", dict(lr=1e-5)), ("ss_reconstructor.", dict(freeze=True))],
                          no_decay_1d=True, lr=1e-4, weight_decay=1e-2)
    index = {id(p): i for i, p in enumerate(gb.params)}
    group_of = [-1] * len(gb.params)
    for k, grp in enumerate(groups):
        for p in grp["params"]:
            group_of[index[id(p)]] = k
    everything = [True] * len(gb.params)
    tags1 = tag_table(gb, [0] * len(gb.params), everything).to(dev)
    tags4 = tag_table(gb, group_of, everything).to(dev)
    table1 = table([(1e-4, 1e-2)])
    table4 = table([(grp["lr"], grp["weight_decay"]) for grp in groups])
    covered4 = 4 * int((tags4 != 0).sum())

    def state():
        return start.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)

    def old(p, m, v):
        check(lib().mesm_adamw_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(tags1), n, None, 0, 0.0, ptr(lr_t), 0.9, 0.999,
                                    1e-8, 1e-2, ptr(step_t), None, stream_ptr()), "mesm_adamw_step")

    def new(tags, tab, n_groups):
        def f(p, m, v):
            check(lib().mesm_adamw_step_groups(ptr(p), ptr(g), ptr(m), ptr(v), ptr(tags), n, None, 0, 0.0, ptr(tab),
                                               n_groups, ptr(step_t), None, stream_ptr()), "mesm_adamw_step_groups")
        return f

    # bytes a launch moves: 28 per updated element, one tag byte per 4 elements of the whole buffer
    forms = [("mesm_adamw_step", old, n), ("step_groups, 1 group", new(tags1, table1, 1), n),
             ("step_groups, %d groups" % len(groups), new(tags4, table4, len(groups)), covered4)]
    runs = [(name, fn, 28 * elems + n // 4, state()) for name, fn, elems in forms]
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
    print("%d elements, %d rounds x %d launches per form" % (n, a.rounds, a.launches))
    for name, _, nbytes, _ in runs:
        t = ms[name]
        med = statistics.median(t)
        res["forms"][name] = {"ms_per_launch_median": med, "ms_per_launch_min": min(t), "ms_per_launch_max": max(t),
                              "spread_rel": (max(t) - min(t)) / med, "bytes_per_launch": nbytes,
                              "GBps_median": nbytes / med / 1e6, "ms_per_launch_rounds": t}
        print("%-24s %.4f ms/launch (min %.4f, max %.4f, spread %.2f%%)  %7.0f GB/s  over %.1f MB"
              % (name, med, min(t), max(t), 100 * (max(t) - min(t)) / med, nbytes / med / 1e6, nbytes / 1e6))
    base = res["forms"]["mesm_adamw_step"]
    for name, _, _, _ in runs[1:2]:
        d = res["forms"][name]["ms_per_launch_median"] / base["ms_per_launch_median"] - 1
        res["one_group_vs_old_rel"] = d
        print("%s against mesm_adamw_step: %+.2f%% (the old entry's own spread: %.2f%%)"
              % (name, 100 * d, 100 * base["spread_rel"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
