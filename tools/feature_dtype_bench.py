"""float32 against float16 video features on one MI355X, alternating the two in ONE process (devices of a pool differ by
several per cent: numbers from two runs do not compare).  Four measurements, one JSON line:

  layernorm     the wide input LayerNorm launches over raw features: 2400 x 2818 plain and twin (one read of x, two outputs
                under two dropout masks), 8192 x 4098 plain; device events around `--reps` launches, every shape warmed up,
                `--rounds` alternations, median
  from_host     C3a and C5: GraphedStep.load_batch(host_batch, redraw=True); run(redraw=False) -- the loop bench.py times
                for `pcie_inclusive_not_in_metric` -- with the host batch's features in either type
  caller        C3a: the unchanged caller, batching.prepare_batch_input(batch, device, feature_dtype=...) + model / criterion
                / backward behind autograph; feature_dtype=None is the float32 path as it always was
  bytes         host bytes a step moves, from the shapes

There is no fallback: without a GPU the tool fails.

    python tools/feature_dtype_bench.py [--steps 30 --warmup 5 --rounds 3 --skip C5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

DTYPES = (("float32", torch.float32), ("float16", torch.float16))


def bench_layernorm(rounds, reps):
    from mesm_amd import kernels as kn
    dev = torch.device("cuda:0")
    cases = [("2400x2818", 2400, 2818, False), ("2400x2818_twin", 2400, 2818, True), ("8192x4098", 8192, 4098, False)]
    out = {}
    for name, rows, D, twin in cases:
        g = torch.Generator().manual_seed(1)
        x32 = torch.randn(rows, D, generator=g).half().float().to(dev)
        xs = {"float32": x32, "float16": x32.half()}
        gam, bet = torch.ones(D, device=dev), torch.zeros(D, device=dev)
        ya, yb = torch.empty(rows * D, device=dev), torch.empty(rows * D, device=dev)

        def launch(x):
            if twin:
                with kn.phase():
                    kn.layernorm_fwd(x, gam, bet, 1e-5, (0.1, 3), out=ya)
                    kn.layernorm_fwd(x, gam, bet, 1e-5, (0.1, 5), out=yb)
            else:
                kn.layernorm_fwd(x, gam, bet, 1e-5, (0.1, 3), out=ya)

        times = {k: [] for k in xs}
        for k in xs:
            for _ in range(5):
                launch(xs[k])
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k in xs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    launch(xs[k])
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / reps * 1e3)
        written = rows * D * 4 * (2 if twin else 1)
        out[name] = {k: {"us_per_launch": statistics.median(v), "rounds_us": v,
                         "bytes_read": rows * D * xs[k].element_size(), "bytes_written": written} for k, v in times.items()}
    return out


def host_bytes(batch):
    return sum(v.numel() * v.element_size() for v in batch.values() if torch.is_tensor(v))


def bench_from_host(workload, steps, warmup, rounds):
    from mesm_amd import build_criterion, build_model, synthetic
    from mesm_amd.graphed import GraphedStep, capture_batch
    dev = torch.device("cuda:0")
    args = synthetic.make_args(workload, device="cuda:0")
    torch.manual_seed(1234)
    model = build_model(args)
    crit = build_criterion(args)
    model.train()
    model.autograph(False)
    res, steps_ = {}, {}
    hosts = {k: synthetic.workload_batch(workload, seed=0, feature_dtype=dt) for k, dt in DTYPES}
    for k, _ in DTYPES:
        steps_[k] = GraphedStep(model, crit, capture_batch(hosts[k], dev), args.dataset_name, warmup=1)
        assert steps_[k].batch["video_feat"].dtype == hosts[k]["video_feat"].dtype
        for _ in range(warmup):
            steps_[k].load_batch(hosts[k], redraw=True)
            steps_[k].run(redraw=False)
    torch.cuda.synchronize()
    times = {k: [] for k, _ in DTYPES}
    for _ in range(rounds):
        for k, _ in DTYPES:
            gs, hb = steps_[k], hosts[k]
            for _ in range(3):
                gs.load_batch(hb, redraw=True)
                gs.run(redraw=False)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(steps):
                gs.load_batch(hb, redraw=True)
                gs.run(redraw=False)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t) / steps * 1e3)
    for k, _ in DTYPES:
        res[k] = {"ms_per_step": statistics.median(times[k]), "rounds_ms": times[k], "host_bytes_per_step": host_bytes(hosts[k]),
                  "video_feat_bytes": hosts[k]["video_feat"].numel() * hosts[k]["video_feat"].element_size()}
    del steps_, model, crit
    torch.cuda.empty_cache()
    return res


def bench_caller(workload, steps, warmup, rounds):
    """prepare_batch_input + the reference's loop body (train.py:64-72 without the optimizer) behind autograph"""
    from mesm_amd import batching, build_criterion, build_model, synthetic
    dev = torch.device("cuda:0")
    args = synthetic.make_args(workload, device="cuda:0")
    torch.manual_seed(1234)
    model = build_model(args)
    crit = build_criterion(args)
    model.train()
    crit.train()
    model.autograph(True)
    host = [synthetic.workload_batch(workload, seed=i) for i in range(4)]

    def one(i, fdt):
        b = batching.prepare_batch_input(dict(host[i % len(host)]), dev, non_blocking=True, feature_dtype=fdt)
        out = model(**b, dataset_name=args.dataset_name, is_training=True)
        _, loss = crit(out, b, is_training=True)
        model.zero_grad(set_to_none=True)
        loss.backward()

    modes = (("float32", None), ("float16", torch.float16))
    for _, fdt in modes:
        for i in range(max(warmup, 3)):
            one(i, fdt)
    torch.cuda.synchronize()
    times = {k: [] for k, _ in modes}
    for _ in range(rounds):
        for k, fdt in modes:
            torch.cuda.synchronize()
            t = time.perf_counter()
            for i in range(steps):
                one(i, fdt)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t) / steps * 1e3)
    auto = model._auto
    return {"counters": {"eager": auto.eager, "captures": auto.captures, "replays": auto.replays},
            **{k: {"ms_per_step": statistics.median(v), "rounds_ms": v} for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--skip", action="append", default=[], help="C5 / caller / layernorm")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("feature_dtype_bench needs an MI355X: there is no CPU path")
    from mesm_amd import synthetic
    report = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds}
    if "layernorm" not in a.skip:
        report["layernorm"] = bench_layernorm(a.rounds, a.reps)
    report["from_host"] = {}
    for wlname in ("C3a", "C5"):
        if wlname in a.skip:
            continue
        report["from_host"][wlname] = bench_from_host(wlname, a.steps, a.warmup, a.rounds)
    if "caller" not in a.skip:
        report["caller"] = {"C3a": bench_caller("C3a", a.steps, a.warmup, a.rounds)}
    report["bytes"] = {}
    for wlname in ("C3a", "C5"):
        w = synthetic.WORKLOADS[wlname]
        n = sum(w["groups"])
        report["bytes"][wlname] = {k: n * w["Lv"] * w["v_feat_dim"] * torch.empty(0, dtype=dt).element_size() for k, dt in DTYPES}
    print(json.dumps(report))


if __name__ == "__main__":
    main()
