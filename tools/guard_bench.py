"""What the non-finite guard (mesm_grad_guard) costs behind the sum of squares and in front of the gated AdamW update, on the
flagship model's flat buffers (C3a: 13.7 M elements, its own segment table).

One process alternates three forms and times each with device events over LAUNCHES tails per round:
(a) mesm_grad_sumsq_gated + mesm_adamw_step_gated on the cycle's due word -- the captured tail as it is without the guard;
(b) the same with mesm_grad_guard between the two and the update gated by the guard's word, on finite gradients: the update
    runs, and the guard reads the partials once per workgroup and ends;
(c) (b) on a gradient buffer that is NaN throughout: the guard walks the buffer and counts every element, the update is
    skipped (so (c) is NOT (a) plus something: it saves the update's 383 MB and pays for the walk).
The yardstick is (a) in the same run, with its own round-to-round spread.

Usage: python tools/guard_bench.py [--rounds 7] [--launches 200]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mesm_amd import build_model, synthetic
from mesm_amd._lib import check, lib, ptr, stream_ptr
from mesm_amd.optim import segment_table


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
    g_ok = 1e-3 * torch.randn(n, device=dev)
    g_nan = torch.full((n,), float("nan"), device=dev)
    table, order = segment_table(gb)
    table, n_seg = table.to(dev), len(order)
    lr_t = torch.full((1,), 1e-4, device=dev, dtype=torch.float32)
    active = torch.ones(n // 4, device=dev, dtype=torch.uint8)
    due = torch.ones(1, device=dev, dtype=torch.int32)
    partials = torch.zeros(1024, device=dev)
    norm = torch.zeros(1, device=dev)

    class State:
        def __init__(self):
            self.p, self.m, self.v = start.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
            self.step = torch.full((1,), 10, device=dev, dtype=torch.int32)
            self.gs = torch.zeros(4, device=dev, dtype=torch.int32)
            self.go = torch.zeros(1, device=dev, dtype=torch.int32)
            self.elems = torch.zeros(n_seg, device=dev, dtype=torch.int64)

    def tail(st, g, guard):
        n_p = ctypes.c_int32(0)
        check(lib().mesm_grad_sumsq_gated(ptr(g), n, ptr(partials), ctypes.byref(n_p), ptr(st.step), ptr(due), stream_ptr()),
              "mesm_grad_sumsq_gated")
        gate = due
        if guard:
            check(lib().mesm_grad_guard(ptr(g), n, ptr(table), n_seg, ptr(partials), n_p.value, ptr(due), ptr(st.step),
                                        ptr(st.gs), ptr(st.go), ptr(norm), ptr(st.elems), stream_ptr()), "mesm_grad_guard")
            gate = st.go
        check(lib().mesm_adamw_step_gated(ptr(st.p), ptr(g), ptr(st.m), ptr(st.v), ptr(active), n, ptr(partials), n_p.value,
                                          0.1, ptr(lr_t), 0.9, 0.999, 1e-8, 1e-2, ptr(st.step), ptr(norm), ptr(gate),
                                          stream_ptr()), "mesm_adamw_step_gated")

    forms = [("(a) sumsq + gated update", g_ok, False), ("(b) + guard, finite gradients", g_ok, True),
             ("(c) + guard, NaN throughout", g_nan, True)]
    runs = [(name, g, guard, State()) for name, g, guard in forms]
    for _, g, guard, st in runs:  # warm-up: code objects, clocks
        for _ in range(20):
            tail(st, g, guard)
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _, _ in runs}
    for _ in range(a.rounds):
        for name, g, guard, st in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                tail(st, g, guard)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.launches)
    # what the counters say the three forms did
    sts = {name: st for name, _, _, st in runs}
    done = a.rounds * a.launches + 20
    assert sts[forms[1][0]].gs.tolist() == [done, 0, 0, 0] and int(sts[forms[1][0]].elems.sum()) == 0
    assert sts[forms[2][0]].gs.tolist() == [done, done, done, done] and int(sts[forms[2][0]].elems.sum()) == done * n
    assert int(sts[forms[2][0]].step) == 10 and int(sts[forms[1][0]].step) == 10 + done
    res = {"elements": n, "segments": n_seg, "rounds": a.rounds, "launches_per_round": a.launches, "forms": {}}
    print("%d elements in %d segments, %d rounds x %d tails per form" % (n, n_seg, a.rounds, a.launches))
    for name, _, _, _ in runs:
        t = ms[name]
        med = statistics.median(t)
        res["forms"][name] = {"us_per_tail_median": 1e3 * med, "us_per_tail_min": 1e3 * min(t), "us_per_tail_max": 1e3 * max(t),
                              "spread_rel": (max(t) - min(t)) / med, "us_per_tail_rounds": [1e3 * x for x in t]}
        print("%-32s %8.2f us/tail (min %.2f, max %.2f, spread %.2f%%)"
              % (name, 1e3 * med, 1e3 * min(t), 1e3 * max(t), 100 * (max(t) - min(t)) / med))
    base = res["forms"][forms[0][0]]
    for name, _, _, _ in runs[1:]:
        d = res["forms"][name]["us_per_tail_median"] - base["us_per_tail_median"]
        res["forms"][name]["vs_a_us"] = d
        print("%s against (a): %+.2f us (the spread of (a) itself: %.2f us)"
              % (name, d, base["us_per_tail_max"] - base["us_per_tail_min"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
