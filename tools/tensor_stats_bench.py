"""What the per-tensor statistics (mesm_tensor_stats) cost between the sum of squares and the gated AdamW update, on the
flagship model's flat buffers (C3a: 13.7 M elements, its own segment table).

One process alternates four forms and times each with device events over LAUNCHES tails per round:
(a) mesm_grad_sumsq_gated + mesm_adamw_step_gated on the cycle's due word -- the captured tail with the switch off;
(b) the same with mesm_tensor_stats between the two and an interval of 1: every tail takes a sample (the launch reads g and
    p once, 2 x 54.7 MB);
(c) (b) with an interval of 100: 99 launches in 100 read three words and end;
(d) a lone mesm_grad_sumsq, for scale: one read of g, half the bytes of a sample.
The yardstick is (a) in the same run, with its own round-to-round spread.

Usage: python tools/tensor_stats_bench.py [--rounds 7] [--launches 200]"""
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
    g = 1e-3 * torch.randn(n, device=dev)
    table, order = segment_table(gb)
    table, n_seg = table.to(dev), len(order)
    n_wg = int(lib().mesm_tensor_stats_workgroups(n))
    lr_t = torch.full((1,), 1e-4, device=dev, dtype=torch.float32)
    active = torch.ones(n // 4, device=dev, dtype=torch.uint8)
    due = torch.ones(1, device=dev, dtype=torch.int32)
    partials = torch.zeros(1024, device=dev)
    norm = torch.zeros(1, device=dev)

    class State:
        def __init__(self, every):
            self.p, self.m, self.v = start.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
            self.step = torch.full((1,), 10, device=dev, dtype=torch.int32)
            self.st = torch.tensor([every or 0, 0, 0, 0], device=dev, dtype=torch.int32)
            self.sumsq = torch.zeros(2 * (n_seg + n_wg), device=dev, dtype=torch.float64)
            self.absmax = torch.zeros(2 * (n_seg + n_wg), device=dev, dtype=torch.int32)

    def tail(st, every):
        n_p = ctypes.c_int32(0)
        if every == "sumsq":
            check(lib().mesm_grad_sumsq(ptr(g), n, ptr(partials), ctypes.byref(n_p), ptr(st.step), stream_ptr()), "mesm_grad_sumsq")
            return
        check(lib().mesm_grad_sumsq_gated(ptr(g), n, ptr(partials), ctypes.byref(n_p), ptr(st.step), ptr(due), stream_ptr()),
              "mesm_grad_sumsq_gated")
        if every:
            check(lib().mesm_tensor_stats(ptr(g), ptr(st.p), n, ptr(table), n_seg, ptr(due), ptr(st.step), ptr(st.st),
                                          ptr(st.sumsq), ptr(st.absmax), stream_ptr()), "mesm_tensor_stats")
        check(lib().mesm_adamw_step_gated(ptr(st.p), ptr(g), ptr(st.m), ptr(st.v), ptr(active), n, ptr(partials), n_p.value,
                                          0.1, ptr(lr_t), 0.9, 0.999, 1e-8, 1e-2, ptr(st.step), ptr(norm), ptr(due),
                                          stream_ptr()), "mesm_adamw_step_gated")

    forms = [("(a) sumsq + gated update", None), ("(b) + tensor stats, every update", 1),
             ("(c) + tensor stats, every 100th", 100), ("(d) a lone sum of squares", "sumsq")]
    runs = [(name, every, State(every if isinstance(every, int) else None)) for name, every in forms]
    for _, every, st in runs:  # warm-up: code objects, clocks
        for _ in range(20):
            tail(st, every)
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in runs}
    for _ in range(a.rounds):
        for name, every, st in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                tail(st, every)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.launches)
    # what the counters say the forms did: steps 11 .. 10 + done, every one or every 100th of them sampled
    done = a.rounds * a.launches + 20
    sts = {name: st for name, _, st in runs}
    assert sts[forms[1][0]].st.tolist() == [1, done, 10 + done, 0]
    assert sts[forms[2][0]].st.tolist() == [100, (10 + done) // 100, (10 + done) // 100 * 100, 0]
    assert all(int(st.step) == 10 + done for st in sts.values())
    res = {"elements": n, "segments": n_seg, "workgroups": n_wg, "rounds": a.rounds, "launches_per_round": a.launches,
           "forms": {}}
    print("%d elements in %d segments, %d rounds x %d tails per form" % (n, n_seg, a.rounds, a.launches))
    for name, _, _ in runs:
        t = ms[name]
        med = statistics.median(t)
        res["forms"][name] = {"us_per_tail_median": 1e3 * med, "us_per_tail_min": 1e3 * min(t), "us_per_tail_max": 1e3 * max(t),
                              "spread_rel": (max(t) - min(t)) / med, "us_per_tail_rounds": [1e3 * x for x in t]}
        print("%-34s %8.2f us/tail (min %.2f, max %.2f, spread %.2f%%)"
              % (name, 1e3 * med, 1e3 * min(t), 1e3 * max(t), 100 * (max(t) - min(t)) / med))
    base = res["forms"][forms[0][0]]
    for name, _, _ in runs[1:3]:
        d = res["forms"][name]["us_per_tail_median"] - base["us_per_tail_median"]
        res["forms"][name]["vs_a_us"] = d
        print("%s against (a): %+.2f us (the spread of (a) itself: %.2f us)"
              % (name, d, base["us_per_tail_max"] - base["us_per_tail_min"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
