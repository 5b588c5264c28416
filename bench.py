"""bench.py — clip-query pairs/s (fwd + criterion + bwd) of the MESM hot path on MI355X.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus N ...          # starts torch.distributed.run itself (before touching a GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A step = model(**batch) -> criterion(outputs, batch) -> zero_grad -> total.backward()
[-> gradient all-reduce of the flat buffer for N > 1: on this library's own RCCL communicator, recorded inside the
step graph, form (one all-reduce in line / six buckets overlapped with backward) chosen by a start-up probe; see
MESM_DDP_MODE], in
TRAIN mode (all dropouts active), on the QVHighlights C+SF workload "C3a" of SURVEY.md 8d (32 pairs per
GPU, Lv=75, Lw=32, Dv=2818, Dt=512, C=5003, fp32).  Inputs are resident in HBM before the timed
region; the host-side draws of the reference (negative query index, MLM word choice) are re-drawn
every step (drawn for step i + 1 while step i runs on the device).  For N > 1 rank r takes the video groups r::N of a global batch of 32 N groups
(mesm_amd.ddp.shard_groups): weak scaling, 32 pairs per GPU.

A plain run sets up, runs the W warm-up steps, times the K steps, writes the outputs of the last timed step when
--dump-outputs DIR is given, and prints the result line: `value` (pairs/s), `ms_per_step`, `dtype` and the step-level
roofline fractions.  Everything else below -- the settled re-timing, host work per step, the dominant kernel family,
`families`, the other arithmetics and workloads, the eager / unchanged-caller / PCIe / loader-like steps, the optimizer
tail, the run-to-run spread and cpu_baseline -- runs only with --full (its fields are null in a plain line).

    python bench.py --gpus 1 --steps 20 --warmup 5 --full
    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR

--dump-outputs DIR: what a caller of the timed step receives after its last replay -- the total loss (`loss.npy`), every
entry of the loss dict (`loss.<name>.npy`) and the gradient (`grad.npy`: every parameter's, concatenated in
named_parameters() order; see dump_outputs), float32, at most 64 MB in all (beyond that each array is the same seeded
sample of its elements in every run).  The inputs are seeded (weights,
batch, host draws, dropout seeds): two runs with the same arguments compute on identical inputs, so two builds can be
compared output for output.

Prints ONE JSON line on rank 0 (contract in the task statement) including
  roofline     — SURVEY 8d's step-level figures: `step_hbm_frac` = algorithmic bytes of the step
                 (0.272 GB + N_pairs x 109.0 MB) / t_step / 8 TB/s and `step_mfma_frac` = N_pairs x 6.22
                 GFLOP / t_step / 157.3 TF; and (--full), as achieved / peak / frac, the dominant kernel family
                 (mesm_gemm_f32: f32 GEMMs whose large products run as three fp16 MFMA products over operands split
                 into two fp16 terms under a wave-owned power-of-two scale, f32 accumulate -- MESM_GEMM_BF16X=6 for
                 round 4's six bf16 products, 0 for f32 MFMA throughout): algorithmic FLOPs per launch / mean launch
                 duration, HIP events on the launch stream around back-to-back replays of the GEMM
                 launches of one captured step, right after the timed region; `traffic` = HBM bytes per
                 launch from the rocprofv3 PMC passes committed under profiles/ (null when that profile
                 was taken with another launch count, i.e. is stale); `families` = in-situ ms per kernel
                 family (GEMM / attention / LayerNorm / losses / element-wise / assembly) by ablation;
                 `attention_hbm_frac` / `layernorm_hbm_frac` = SURVEY 8d's byte split / family ms / 8 TB/s;
                 `exact_f32` / `exact_f32_ms` / `bf16x6` = the same step with every product on the f32 MFMA instruction /
                 in round 4's six-product bf16 split (child processes of this run);
                 `deterministic_ms_per_step` / `run_to_run_grad_spread` = the step with MESM_GEMM_FWD_ATOMICS=0 (bit-
                 reproducible loss) and the gradient spread between two replays of one batch in either setting;
  config       — besides the workload: `ddp`, and (not part of the metric) the eager step, `unchanged_caller_ms_per_step`
                 (the reference's loop body train.py:64-72 verbatim -- model(**batch), criterion(...), zero_grad, backward,
                 torch's clip_grad_norm_ and AdamW.step -- on graph replays behind that call sequence, mesm_amd/autograph.py),
                 `other_workloads_not_in_metric` (C2 / C3b / C5 step times with their roofline fractions), the optimizer tail, the
                 PCIe-inclusive rate, and `loader_like_epoch_not_in_metric`: a stream of loader-shaped batches
                 from host memory through StepCache (pair axis padded, real count on the device);
  cpu_baseline — (--full) the CPU oracle (a port of the reference step, oracle/mesm_oracle.py) timed on
                 this box's host cores on the same workload, train mode (rank 0, N = 1 only): 2 warm-up
                 steps, median of 5.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_BF16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA peak (v_mfma_f32_32x32x16_bf16)


def gemm_mode():
    """the GEMM arithmetic of this process, as the loaded library reports it (MESM_GEMM_BF16X is read once at load and
    tools may change it through mesm_gemm_set_switches: the environment is not the authority)"""
    from mesm_amd._lib import lib
    return int(lib().mesm_gemm_get_bf16x())


def dtype_name():
    return {6: "f32 (3-term split-bf16 products, f32 accumulate)", 0: "f32",
            2: "f32 (2-term split-fp16 products under a wave-owned power-of-two scale, 3 MFMA products, f32 accumulate)"}[gemm_mode()]


def draws_mode():
    from mesm_amd import draws
    return ("%s (mesm_amd/draws.py; host_ms_per_step = host work of one step: graph launch call + the next step's "
            "negative / masked-word draws + their upload, measured with the device idle at the start of the step so that no "
            "back-pressure wait is counted; in the timed loop it overlaps the device step)" % draws.MODE)


SETTLE_STEPS = 60  # untimed steps in front of the SECOND, informational timing (config.settled: not the headline)
PEAK_HBM_TBS = 8.0            # MI355X_MICROARCH.md: HBM3E spec peak
# algorithmic work of one step (kernel-boundary traffic / FLOPs); closed form for C3a-type batches,
# the analytic model's totals for the other workloads
STEP_WORK = {"C1": (0.48e9, 12.0e9), "C2": (3.49e9, 183.7e9), "C3b": (5.07e9, 257.9e9), "C5": (10.83e9, 646.2e9)}


def step_work(workload, n_pairs):
    if workload in STEP_WORK:
        return STEP_WORK[workload]
    return 0.272e9 + n_pairs * 109.0e6, n_pairs * 6.22e9


DUMP_BYTES = 64 * 10 ** 6  # --dump-outputs: all files together (the C3a gradient alone is 55 MB)


def dump_outputs(path, total, losses, model):
    """--dump-outputs: what the last step hands its caller, as float32 .npy files: the total loss (loss.npy), every entry
    of the loss dict (loss.<name>.npy) and the gradient (grad.npy): every parameter's .grad flattened and concatenated
    in model.named_parameters() order, zeros for a parameter without one.  The gradient is ONE array because it is one
    vector to its caller (param.grad are views of one flat buffer; clip_grad_norm_, the optimizer and the all-reduce act
    on all of it), and because some of its parameters have an exactly zero gradient -- the key-projection biases: softmax
    does not see a shift shared by every key -- where the kernels' float atomics leave summation noise that differs from
    run to run and is rounding only at the scale of the whole gradient.  If the files would not fit in DUMP_BYTES, every
    array is cut down to the same fraction of its elements, picked by a fixed seed (the same elements in every run)."""
    import numpy as np
    import torch
    arrays = {"loss": total}
    arrays.update(("loss." + k, v) for k, v in losses.items())
    arrays["grad"] = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1)
                                for _, p in model.named_parameters()])
    arrays = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    keep = min(1.0, (DUMP_BYTES - 256 * len(arrays)) / sum(a.nbytes for a in arrays.values()))  # (256: .npy header)
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        if keep < 1.0 and a.size > 1:
            idx = np.random.RandomState(0).choice(a.size, max(1, int(a.size * keep)), replace=False)
            a = a.reshape(-1)[np.sort(idx)]
        np.save(os.path.join(path, k + ".npy"), a)
    log("outputs of the last timed step: %d arrays in %s" % (len(arrays), path))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="C3a")
    ap.add_argument("--cpu-steps", type=int, default=5, help="timed oracle steps for cpu_baseline (0 = skip; --full only)")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the informational sections (profiling runs)")
    ap.add_argument("--eager", action="store_true", help="launch every kernel from Python (no HIP graph)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run every informational measurement and check (see the module docstring)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the loss entries and gradients of the last timed step to DIR/<name>.npy")
    return ap.parse_args()


def log(msg):
    print("[bench %8.2fs] %s" % (time.perf_counter() - T_START, msg), file=sys.stderr, flush=True)


T_START = time.perf_counter()


def host_cores():
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    # respect a cgroup CPU quota if there is one
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = max(1, min(n, int(float(q) / float(per))))
    except (OSError, ValueError):
        pass
    return n


def spawn_ranks(opt):
    """`python bench.py --gpus N` without a torchrun environment: start one rank per GPU as CHILD processes
    (this parent never initialises a GPU and never re-execs) and pass rank 0's JSON line through."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(opt.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run(cmd, env=env)
    raise SystemExit(r.returncode)


_WATCHDOG = {"armed": False, "line": None}


def _watchdog_fire():
    """a stalled own-communicator diagnostic must not cost the run its (already measured) headline"""
    if not _WATCHDOG["armed"]:
        return
    sys.stderr.write("[bench] own-communicator diagnostics did not finish in time: reporting the `after` headline\n")
    if _WATCHDOG["line"] is not None:
        print(json.dumps(_WATCHDOG["line"]), flush=True)
    sys.stdout.flush()
    sys.stderr.flush()
    # the `after` headline above is a complete, measured line -- but a stalled collective is NOT a clean run: leave with a
    # non-zero status so that the launcher sees it; never restart or re-exec from here (the GPU is initialised)
    os._exit(3)


def ddp_diagnostics(opt, world, rank, dev, model, crit, batch, args, g_after, r_after, diag, fence, n_pairs, t_after,
                    force_ddp):
    """After the `after` headline: the library's own RCCL communicator (never run on > 1 rank before round 4) built,
    counted, and VERIFIED (exact all-reduce of integer-valued data on both issue paths; after a step of either captured
    form every rank holds the same gradient buffer) and its two captured forms TIMED (5 replays, MAX over ranks) next to `after`.  Fills `diag`; returns (name, (graphed step, reducer)) of a
    verified form that beat `after` in the probe, else (None, None).  Every rank arms a watchdog first: if anything in
    here stalls (a collective that never completes), rank 0 prints the `after` headline and every rank leaves."""
    import threading
    import torch
    import torch.distributed as dist
    from mesm_amd.ddp import GradReducer, RcclComm, ranks_agree
    from mesm_amd.graphed import GraphedStep
    limit = float(os.environ.get("MESM_BENCH_DIAG_TIMEOUT", "180"))
    if rank == 0:
        _WATCHDOG["line"] = {
            "metric": "clip-query pairs/sec (fwd+bwd)", "value": n_pairs * world / t_after, "unit": "pairs/s",
            "n_gpus": world, "steps": opt.steps, "warmup": opt.warmup, "ms_per_step": t_after * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": dtype_name(), "data": "synthetic",
            "config": {"workload": opt.workload, "global_pairs": n_pairs * world, "parallelism": "dp%d" % world,
                       "launch": "hip-graph",
                       "ddp": "torch process group: one blocking all-reduce of the flat buffer after the graph replay "
                              "(own-communicator diagnostics timed out after %.0f s)" % limit,
                       "ddp_diag": dict(diag, timed_out=True)},
            "roofline": _WATCHDOG.get("roofline"), "cpu_baseline": _WATCHDOG.get("cpu_baseline")}
    _WATCHDOG["armed"] = True
    timer = threading.Timer(limit, _watchdog_fire)
    timer.daemon = True
    timer.start()
    gb = model.gradbuf()

    def reduced(run):  # the flat gradient buffer after one step of a form, same batch, same draws
        run()
        torch.cuda.synchronize()
        return gb.flat.detach().clone()

    def after_step():
        g_after.run(redraw=False)
        r_after.finish()

    def timed(run):
        for _ in range(2):
            run()
        fence()
        p0 = time.perf_counter()
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        pt = torch.tensor([(time.perf_counter() - p0) / 5 * 1e3], device=dev, dtype=torch.float64)
        if world > 1:
            dist.all_reduce(pt, op=dist.ReduceOp.MAX)
        return float(pt.item())

    diag["probe_ms"] = {"after": timed(after_step)}
    got = reduced(after_step)
    same, spread = ranks_agree(got)
    diag["grad_checksum_spread_by_form"] = {"after": spread}  # (`grad_checksum_spread_over_ranks`: the headline form's)
    diag["after_ranks_agree"] = bool(same)
    diag["_after_objs"] = (g_after, r_after, True)
    best, own = None, None
    ok = 1
    cands = {}
    try:
        if os.environ.get("MESM_BENCH_FAIL_OWN") == "1":  # (exercises the failure path)
            raise RuntimeError("simulated failure of the own-communicator path")
        comm = RcclComm(dev)
        diag["rccl_ranks"] = comm.count()
        for c in ("own-inline", "own-overlapped"):
            inl = c == "own-inline"
            red = GradReducer(gb, hook=True, inline=inl, n_buckets=1 if inl else 6, comm=comm, fold_scale=True,
                              force=force_ddp)
            cands[c] = (GraphedStep(model, crit, batch, args.dataset_name, reducer=red), red)
    except Exception as e:  # noqa: BLE001
        diag["own_communicator_error"] = "%s: %s" % (type(e).__name__, str(e)[:200])
        ok = 0
    gb.on_ready = None  # (the candidates' reducers hooked themselves in for their captures)
    if world > 1:  # every rank has to have every candidate before any of their collectives is replayed
        flag = torch.tensor([ok], device=dev, dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        ok = int(flag.item())
    if ok:
        # (1) the communicator itself, outside any graph: exact sums of integer-valued data on both issue paths
        n = (1 << 20) + 3
        basev = (torch.arange(n, device=dev) % 251).float()
        want = basev * (world * (world + 1) // 2)
        exact = True
        for side in (False, True):
            t = basev * (rank + 1)
            comm.allreduce(t, side=side)
            if side:
                comm.wait()
            torch.cuda.synchronize()
            exact = exact and bool(torch.equal(t, want))
        ex = torch.tensor([1 if exact else 0], device=dev, dtype=torch.int32)
        if world > 1:
            dist.all_reduce(ex, op=dist.ReduceOp.MIN)
        diag["own_comm_selftest_exact"] = bool(int(ex.item()))
        # (2) every captured form: after one step all ranks hold the same gradient buffer (dropout masks differ from
        # replay to replay, so the forms cannot be compared with each other value by value), then (3) its time
        diag["own_forms_ranks_agree"] = {}
        for c, (gs, red) in cands.items():
            got = reduced(lambda gs=gs: gs.run(redraw=False))
            same, spread = ranks_agree(got)
            fin = bool(torch.isfinite(got).all())
            diag["own_forms_ranks_agree"][c] = {"ranks_agree": bool(same), "checksum_spread": spread, "finite": fin}
            diag["grad_checksum_spread_by_form"][c] = spread
            verified = diag["own_comm_selftest_exact"] and same and fin
            if not verified:
                diag.setdefault("refused_forms", []).append(c)
            if diag["own_comm_selftest_exact"]:
                # timed even when refused (the first real N > 1 line shows all three timings); only a
                # verified form can become the headline
                diag["probe_ms"][c] = timed(lambda gs=gs: gs.run(redraw=False))
        good = {k: v for k, v in diag["probe_ms"].items() if k != "after" and k not in diag.get("refused_forms", [])}
        if good:
            b = min(good, key=good.get)
            if good[b] < diag["probe_ms"]["after"] * 0.99:
                best, own = b, cands[b]
    timer.cancel()
    if best is None:
        _WATCHDOG["armed"] = False
    else:  # the re-timing of the chosen form in main() stays under a fresh watchdog (its line says which form stalled)
        if rank == 0 and _WATCHDOG["line"] is not None:
            _WATCHDOG["line"]["config"]["ddp_diag"] = dict(diag, timed_out=True, timed_out_while="re-timing " + best)
            _WATCHDOG["line"]["config"]["ddp_diag"].pop("_after_objs", None)
        t2 = threading.Timer(limit, _watchdog_fire)
        t2.daemon = True
        t2.start()
    return best, own


def main():
    opt = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1 and opt.gpus > 1:
        spawn_ranks(opt)
    import torch
    from mesm_amd import build_criterion, build_model, synthetic
    from mesm_amd import kernels as kn
    from mesm_amd.ddp import GradReducer, init_process_group_from_env, shard_groups

    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if opt.gpus != world:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (opt.gpus, world))
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    import torch.distributed as dist
    if world > 1:
        init_process_group_from_env(dev)

    wl = dict(synthetic.WORKLOADS[opt.workload])
    args = synthetic.make_args(opt.workload, device=str(dev))
    torch.manual_seed(1234)  # identical weights on every rank
    model = build_model(args)
    crit = build_criterion(args)
    model.train()
    model.autograph(False)  # this script drives its graphs itself; `unchanged_caller` below switches it on for its loop
    from mesm_amd.graphed import GraphedStep

    if world > 1:
        # one global batch of world x the workload's groups, sharded by video group r::W
        wg = dict(wl)
        gl = synthetic.make_batch(wg["dataset_name"], wg["groups"] * world, wg["Lv"], wg["Lw"], wg["v_feat_dim"],
                                  wg["t_feat_dim"], wg["vocab_size"] + 1, seed=0)
        batch_cpu = shard_groups(gl, rank, world)
        del gl
    else:
        batch_cpu = synthetic.workload_batch(opt.workload, seed=0)
    batch = synthetic.to_device(batch_cpu, dev)
    n_pairs = batch_cpu["video_feat"].shape[0]
    torch.manual_seed(99 + rank)  # per-rank host-RNG streams (negatives, MLM words), SURVEY 8e
    import numpy as _np
    _np.random.seed(99 + rank)    # (the vectorized draws read numpy's global stream, mesm_amd/draws.py)

    eager_losses = {}

    def eager_step():
        out = model(**batch, dataset_name=args.dataset_name, is_training=True)
        losses, total = crit(out, batch, True)
        model.zero_grad(set_to_none=True)
        total.backward()  # the reducer's finish() runs as an engine callback for world > 1
        eager_losses.update(losses)
        return total

    ddp_mode = None
    if opt.eager:
        reducer = GradReducer(model.gradbuf()) if world > 1 else None
        step = eager_step
        ddp_mode = "hooks-from-backward (eager)" if world > 1 else None
    else:
        # one HIP graph per step: forward + criterion + backward; fresh host draws + dropout masks every replay.
        # N > 1, MESM_DDP_MODE =
        #   auto (default):  this library's OWN RCCL communicator (csrc/ddp.hip; no process-group watchdog next to the
        #                    captured collectives), the 1 / N of the gradient mean folded into the loss gradient, and a
        #                    start-up PROBE (before the timed region) of the two captured forms -- `own-inline`: one
        #                    all-reduce of the flat buffer recorded at the end of the step graph on the compute stream
        #                    (one queue, wire time exposed); `own-overlapped`: six buckets recorded on the
        #                    communicator's stream from inside backward (wire time hidden, a second hardware queue is
        #                    active: DESIGN.md section 5) -- keeps the faster one (max over ranks);
        #   own-inline / own-overlapped: that form without the probe;
        #   after:           torch.distributed: ONE blocking all-reduce on the compute stream after the graph replay
        #                    (nothing captured; the round-2 default);  captured / inline / after-async: the torch
        #                    process-group forms of round 2.
        gstep, reducer, post = None, None, False
        # default for N > 1: "safe" (no form of the own-communicator path has ever run on more than one rank):
        # the HEADLINE is first measured with `after` (torch process group, nothing captured -- the plain, known-good
        # form); only then, under a watchdog that prints that headline and leaves if anything stalls, the library's own
        # communicator is built, its two captured forms are checked against `after` (same reduced gradients) and timed,
        # and the faster, verified form is re-timed under the full protocol and reported -- with all three side by side
        # in config.ddp_diag.  See ddp_diagnostics() below.
        mode = os.environ.get("MESM_DDP_MODE", "safe")
        force_ddp = os.environ.get("MESM_BENCH_FORCE_DDP") == "1"  # exercise the N > 1 code on one GPU (1-rank groups)
        ddp_on = world > 1 or force_ddp
        safe = ddp_on and mode == "safe"
        if safe:
            mode = "after"
        if ddp_on and mode in ("auto", "own-inline", "own-overlapped"):
            from mesm_amd.ddp import RcclComm
            ok, comm, cands = 1, None, {}
            try:
                if os.environ.get("MESM_BENCH_FAIL_OWN") == "1":  # (exercises the fallback below)
                    raise RuntimeError("simulated failure of the own-communicator path")
                comm = RcclComm(dev)
                for c in (["own-inline", "own-overlapped"] if mode == "auto" else [mode]):
                    inl = c == "own-inline"
                    red = GradReducer(model.gradbuf(), hook=True, inline=inl, n_buckets=1 if inl else 6, comm=comm,
                                      fold_scale=True, force=force_ddp)
                    gs = GraphedStep(model, crit, batch, args.dataset_name, reducer=red)
                    cands[c] = (gs, red)
            except Exception as e:
                log("own-communicator capture failed on this rank (%s: %s)" % (type(e).__name__, e))
                ok = 0
            any_ok = ok
            if world > 1:  # every rank has to agree before anything else is issued (ADVICE: no asymmetric fallback)
                flag = torch.tensor([ok, -ok], device=dev, dtype=torch.int32)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                ok, any_ok = int(flag[0].item()), -int(flag[1].item())
            if not ok and not any_ok:
                # EVERY rank failed the same way (no librccl to dlopen, capture refused, ...): nothing of the own
                # communicator is in flight anywhere, so the plain form is safe to fall back to
                log("own-communicator path unavailable on every rank: falling back to MESM_DDP_MODE=after")
                cands.clear()
                model.gradbuf().on_ready = None  # (the failed candidates' reducers hooked themselves in)
                mode = "after"
            elif not ok:
                raise SystemExit("bench: the captured data-parallel step could not be built on every rank; "
                                 "restart with MESM_DDP_MODE=after")
            probe = {}
            for c, (gs, red) in (cands.items() if ok else ()):
                for _ in range(2):
                    gs.run(redraw=False)
                torch.cuda.synchronize()
                if world > 1:
                    dist.barrier()
                p0 = time.perf_counter()
                for _ in range(5):
                    gs.run(redraw=False)
                torch.cuda.synchronize()
                pt = torch.tensor([(time.perf_counter() - p0) / 5 * 1e3], device=dev, dtype=torch.float64)
                if world > 1:
                    dist.all_reduce(pt, op=dist.ReduceOp.MAX)
                probe[c] = float(pt.item())
            best = min(probe, key=probe.get) if probe else None
            if best is not None:
                gstep, reducer = cands[best]
            cands.clear()
            what = {"own-inline": "one all-reduce of the flat gradient buffer recorded at the end of the step graph on the "
                                  "compute stream (one queue, wire time exposed)",
                    "own-overlapped": "six bucket all-reduces recorded inside the step graph on the communicator's own "
                                      "stream, overlapped with backward"}.get(best)
            if best is not None:
                ddp_mode = ("own RCCL communicator (mesm_ddp_*), 1/N folded into the loss gradient; %s; start-up probe, "
                            "ms/step max over ranks: %s -> %s%s"
                            % (what, ", ".join("%s %.3f" % kv for kv in sorted(probe.items())), best,
                               "" if mode == "auto" else " (forced by MESM_DDP_MODE)"))
        elif ddp_on and mode in ("captured", "inline"):
            ok = 1
            try:
                reducer = GradReducer(model.gradbuf(), hook=True, inline=mode == "inline",
                                      n_buckets=1 if mode == "inline" else 6)
                gstep = GraphedStep(model, crit, batch, args.dataset_name, reducer=reducer)
                ddp_mode = ("torch process group: one all-reduce captured in line at the end of the step graph"
                            if mode == "inline" else
                            "torch process group: bucketed all-reduce captured in the step graph, overlapped with backward")
            except Exception as e:
                log("captured all-reduce failed (%s: %s)" % (type(e).__name__, e))
                ok = 0
            flag = torch.tensor([ok], device=dev, dtype=torch.int32)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if int(flag.item()) == 0:
                raise SystemExit("bench: the captured collectives could not be built on every rank; restart with "
                                 "MESM_DDP_MODE=after")
        if gstep is None:
            gstep = GraphedStep(model, crit, batch, args.dataset_name)
            if ddp_on:
                blocking = mode != "after-async"
                reducer = GradReducer(model.gradbuf(), hook=False, inline=blocking, n_buckets=1 if blocking else 6)
                post = True
                ddp_mode = ("torch process group: one blocking all-reduce of the flat buffer on the compute stream after "
                            "the graph replay" if blocking else
                            "torch process group: asynchronous all-reduces on the collective stream after the graph replay")
        log("step captured in a HIP graph")

        def step():
            # the host half of a step is software-pipelined like a loader's prefetch: replay with the draws prepared
            # during the PREVIOUS step (the very first ones at construction), then draw the next step's while this one
            # runs on the device.  Still one fresh set of host draws per step, K draws inside the K timed steps -- but
            # the device does not idle for the ~1 ms of host RNG work in front of the first timed replay (at K = 20 that
            # idle millisecond was 50 us per step of the round-3 headline).
            total = gstep.run(redraw=False)
            if post:
                reducer.finish()
            gstep.redraw()
            return total

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    log("model built (%d params), starting warm-up" % sum(p.numel() for p in model.parameters()))
    # EXACTLY the W warm-up steps the caller asked for, then EXACTLY K timed steps between two fences: the headline.
    for i in range(opt.warmup):
        step()
        if i == 0:
            torch.cuda.synchronize()
            log("first step done")
    fence()
    log("warm-up done")
    t0 = time.perf_counter()
    for _ in range(opt.steps):
        last = step()
    fence()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    assert torch.isfinite(last), "non-finite loss in the timed region"
    t_step = dt / opt.steps
    log("timed region: %.3f ms/step" % (t_step * 1e3))

    def dump():  # before anything else runs the step again
        if opt.dump_outputs and rank == 0:
            dump_outputs(opt.dump_outputs, last, eager_losses if opt.eager else gstep.losses, model)
    dump()

    # the step-level roofline figures exist as soon as the headline does: a watchdog line (diagnostics that stall) carries them
    _sb, _sf = step_work(opt.workload, n_pairs)
    _WATCHDOG["roofline"] = {"bound": "mfma", "achieved": None, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": None,
                             "traffic": None, "step_hbm_frac": _sb / t_step / (PEAK_HBM_TBS * 1e12),
                             "step_mfma_frac": _sf / t_step / (PEAK_F32_MFMA_TFLOPS * 1e12), "step_bytes": _sb, "step_flops": _sf,
                             "note": "dominant-kernel figures and the CPU baseline are single-GPU measurements (N = 1 run)"}
    ddp_diag = None
    if not opt.eager and ddp_on:
        from mesm_amd.ddp import ranks_agree
        ok_sum, spread = ranks_agree(model.gradbuf().flat)
        ddp_diag = {"world": world, "grad_checksum_spread_over_ranks": spread, "headline_form": mode,
                    "after_ms_per_step": t_step * 1e3 if mode == "after" else None}
        if not ok_sum:
            raise SystemExit("bench: after a data-parallel step the ranks hold DIFFERENT gradient buffers (relative "
                             "checksum spread %.3e): the all-reduce did not do its job" % spread)
    if not opt.eager and safe:
        best, own = ddp_diagnostics(opt, world, rank, dev, model, crit, batch, args, gstep, reducer, ddp_diag, fence,
                                    n_pairs, t_step, force_ddp)
        if best is not None:  # a verified own-communicator form beat `after` in the probe: the full protocol again, on it
            gstep, reducer, post = own[0], own[1], False
            for _ in range(opt.warmup):
                step()
            fence()
            t0 = time.perf_counter()
            for _ in range(opt.steps):
                last = step()
            fence()
            dt2 = time.perf_counter() - t0
            if world > 1:
                t = torch.tensor([dt2], device=dev, dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                dt2 = float(t.item())
            assert torch.isfinite(last), "non-finite loss in the timed region"
            ddp_diag["headline_form"] = best
            ddp_diag[best + "_ms_per_step"] = dt2 / opt.steps * 1e3
            if dt2 / opt.steps < t_step:
                t_step = dt2 / opt.steps
                dump()
                ddp_mode = ("own RCCL communicator (mesm_ddp_*, %d ranks by ncclCommCount), 1/N folded into the loss gradient, "
                            "form %s recorded in the step graph; verified against and faster than `after` (config.ddp_diag)"
                            % (ddp_diag.get("rccl_ranks", -1), best))
            else:
                ddp_diag["headline_form"] = "after"
                gstep, reducer, post = ddp_diag.pop("_after_objs")
            log("timed region (%s): %.3f ms/step" % (best, dt2 / opt.steps * 1e3))
        ddp_diag.pop("_after_objs", None)
        _WATCHDOG["armed"] = False

    # Informational, NOT the headline (round-3 review: the settle steps used to sit in front of the caller's warm-up):
    # the same K steps again after SETTLE_STEPS more untimed ones (a fresh box's first second of replays runs a few
    # percent slow), and the HIP-event MEDIAN per step of BASELINE.md section 4 (one event pair per step on the step's
    # stream, outside the timed region so that no event record sits inside it).
    settled = None
    if opt.full and not opt.eager:
        for _ in range(SETTLE_STEPS):
            step()
        fence()
        t1 = time.perf_counter()
        for _ in range(opt.steps):
            step()
        fence()
        sdt = time.perf_counter() - t1
        evs = []
        for _ in range(opt.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step()
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        ems = sorted(a.elapsed_time(b) for a, b in evs)
        st = torch.tensor([sdt / opt.steps * 1e3, ems[len(ems) // 2]], device=dev, dtype=torch.float64)
        if world > 1:
            dist.all_reduce(st, op=dist.ReduceOp.MAX)
        settled = {"settle_steps": SETTLE_STEPS, "ms_per_step_after_settling": float(st[0].item()),
                   "hip_event_median_ms_per_step": float(st[1].item()),
                   "note": "second timing of the same K steps after settle_steps more untimed steps, and the per-step "
                           "HIP-event median (max over ranks); neither is `value`"}
        log("settled: %.3f ms/step, event median %.3f" % (settled["ms_per_step_after_settling"],
                                                          settled["hip_event_median_ms_per_step"]))

    # HOST work of one step (informational): the same step() with the device idle at its start, so that nothing in it
    # waits for an earlier replay (in the timed loop the arena upload's back-pressure -- at most two steps ahead of
    # the device -- makes step() LAST as long as the device step; that wait is not host work)
    host_ms = None
    if opt.full and not opt.eager:
        hs = 0.0
        for _ in range(opt.steps):
            torch.cuda.synchronize()
            h0 = time.perf_counter()
            step()
            hs += time.perf_counter() - h0
        torch.cuda.synchronize()
        host_ms = hs / opt.steps * 1e3
        log("host work per step %.3f ms" % host_ms)

    extras = opt.full and rank == 0 and not opt.no_extras
    # the fallback path of ragged / unseen batch shapes before their graph exists: every launch from Python
    eager_ms = None
    if extras and not opt.eager and world == 1:
        # on the stream the graphs were captured on, like the warm-up steps of a capture and StepCache's first visit of a
        # shape bucket: autograd pins every AccumulateGrad node to the stream of its first use, and eager steps on ANOTHER
        # stream pay a cross-stream synchronisation per parameter (what rounds 3-4 reported here: 21 / 27 ms)
        from mesm_amd.graphed import capture_stream
        side = capture_stream(dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                eager_step()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(5):
                eager_step()
            torch.cuda.synchronize()
            eager_ms = (time.perf_counter() - t1) / 5 * 1e3
        torch.cuda.current_stream().wait_stream(side)

    # The reference's loop body, train.py:64-72, VERBATIM on the caller's stream with torch's own optimizer and clipping:
    # the first visit of the shape runs eager, the second captures, from the third on every call is a graph replay
    # (mesm_amd/autograph.py).  lr = 0 so that the later sections of this script see unchanged weights (the kernels of
    # AdamW.step run all the same).  The batch is device-resident like after prepare_batch_input.
    unchanged = None
    if extras and not opt.eager and world == 1:
        try:
            from torch import nn
            model.autograph(True)
            ref_opt = torch.optim.AdamW(model.parameters(), lr=0.0, weight_decay=1e-4)

            last_losses = [None]

            def loop_body():
                outputs = model(**batch, dataset_name=args.dataset_name, is_training=True)
                loss_dict, loss = crit(outputs, batch, is_training=True)
                last_losses[0] = loss_dict
                ref_opt.zero_grad()
                loss.backward()
                nn.utils.clip_grad_norm_(model.parameters(), 0.1)
                ref_opt.step()
                return outputs, loss
            for _ in range(6):
                outputs, loss = loop_body()
            torch.cuda.synchronize()
            reps = []
            for _ in range(3):  # (a host-bound sequence: median of three timed runs of K steps)
                t1 = time.perf_counter()
                for _ in range(opt.steps):
                    loop_body()
                torch.cuda.synchronize()
                reps.append((time.perf_counter() - t1) / opt.steps * 1e3)
            uc = sorted(reps)[1]
            t1 = time.perf_counter()
            wd = crit.weight_dict
            for _ in range(opt.steps):
                _, loss = loop_body()
                # train.py:75-77: the reference's logging reads the loss and EVERY entry of the loss dict, every step
                # (the entries share one host fetch: criterion.LossEntry)
                ld = dict(last_losses[0])
                ld["loss_overall"] = float(loss)
                for k_, v_ in ld.items():
                    float(v_) * wd[k_] if k_ in wd else float(v_)
            torch.cuda.synchronize()
            uc_sync = (time.perf_counter() - t1) / opt.steps * 1e3
            t1 = time.perf_counter()
            for _ in range(opt.steps):
                outputs = model(**batch, dataset_name=args.dataset_name, is_training=True)
                loss_dict, loss = crit(outputs, batch, is_training=True)
                ref_opt.zero_grad()
                loss.backward()
            torch.cuda.synchronize()
            uc_fb = (time.perf_counter() - t1) / opt.steps * 1e3
            # the same loop on a batch whose collate kept the host copies of its small tensors (batching.attach_host_side: one
            # line in the DataLoader's collate_fn): the forward needs no transfer back and no synchronisation
            from mesm_amd import batching as _bt
            hbatch = synthetic.to_device(_bt.attach_host_side(dict(batch_cpu)), dev)
            keep = batch
            try:
                batch = hbatch
                for _ in range(3):
                    loop_body()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(opt.steps):
                    loop_body()
                torch.cuda.synchronize()
                uc_host = (time.perf_counter() - t1) / opt.steps * 1e3
            finally:
                batch = keep
            # the same loop with ONE more changed line: `optimizer = mesm_amd.build_optimizer(opt, model)` (FlatAdamW: global-
            # norm clip + AdamW over the flat buffers, two launches) whose step(grad_clip=...) replaces lines 70-72
            from mesm_amd.optim import FlatAdamW
            flat_opt = FlatAdamW(model, lr=0.0, weight_decay=1e-4)
            for _ in range(2):
                outputs = model(**batch, dataset_name=args.dataset_name, is_training=True)
                loss_dict, loss = crit(outputs, batch, is_training=True)
                flat_opt.zero_grad()
                loss.backward()
                flat_opt.step(grad_clip=0.1)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(opt.steps):
                outputs = model(**batch, dataset_name=args.dataset_name, is_training=True)
                loss_dict, loss = crit(outputs, batch, is_training=True)
                flat_opt.zero_grad()
                loss.backward()
                flat_opt.step(grad_clip=0.1)
            torch.cuda.synchronize()
            uc_flat = (time.perf_counter() - t1) / opt.steps * 1e3
            # ... and the loop body LITERALLY unchanged with the optimizer of this build's third factory: train.py:17-18 import
            # build_model, build_criterion AND build_optimizer from runner -- with all three from mesm_amd, `optimizer` is the
            # flat AdamW and lines 64-72 (torch's clip_grad_norm_ included) run as they stand
            for _ in range(2):
                outputs = model(**batch, dataset_name=args.dataset_name, is_training=True)
                loss_dict, loss = crit(outputs, batch, is_training=True)
                flat_opt.zero_grad()
                loss.backward()
                nn.utils.clip_grad_norm_(model.parameters(), 0.1)
                flat_opt.step()
            torch.cuda.synchronize()
            reps3 = []
            for _ in range(3):
                t1 = time.perf_counter()
                for _ in range(opt.steps):
                    outputs = model(**batch, dataset_name=args.dataset_name, is_training=True)
                    loss_dict, loss = crit(outputs, batch, is_training=True)
                    flat_opt.zero_grad()
                    loss.backward()
                    nn.utils.clip_grad_norm_(model.parameters(), 0.1)
                    flat_opt.step()
                torch.cuda.synchronize()
                reps3.append((time.perf_counter() - t1) / opt.steps * 1e3)
            uc_three = sorted(reps3)[1]
            del flat_opt
            a = model._auto
            unchanged = {"ms_per_step": uc, "ms_per_step_three_runs": reps,
                         "ms_per_step_with_the_loops_float_of_every_loss_entry": uc_sync,
                         "with_this_builds_optimizer_step_instead_of_clip_and_torch_adamw_ms": uc_flat,
                         "with_host_side_kept_by_the_collate_ms": uc_host,
                         "loop_body_unchanged_with_all_three_factories_from_this_build_ms": uc_three,
                         "fwd_criterion_zero_grad_backward_only_ms": uc_fb,
                         "pairs_per_s": n_pairs / (uc * 1e-3), "replayed": outputs._auto_step is not None,
                         "eager_visits": a.eager, "captures": a.captures, "replays": a.replays,
                         "sequence": "train.py:64-72: model(**batch) / criterion(outputs, batch) / optimizer.zero_grad() / "
                                     "loss.backward() / nn.utils.clip_grad_norm_ / torch.optim.AdamW.step (lr = 0)"}
            log("unchanged caller: %.3f ms/step (%.3f with the loop's float() of every loss, %.3f without clip + step, %.3f with FlatAdamW.step)"
                % (uc, uc_sync, uc_fb, uc_flat))
        except Exception as e:
            unchanged = {"error": "%s: %s" % (type(e).__name__, e)}
        finally:
            model.autograph(False)
            model.zero_grad(set_to_none=True)

    roofline = {"bound": "mfma", "achieved": None, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": None,
                "traffic": None}
    # SURVEY 8d step-level definition (per rank: every rank runs the same per-GPU workload)
    sbytes, sflops = step_work(opt.workload, n_pairs)
    roofline["step_hbm_frac"] = sbytes / t_step / (PEAK_HBM_TBS * 1e12)
    roofline["step_mfma_frac"] = sflops / t_step / (PEAK_F32_MFMA_TFLOPS * 1e12)
    roofline["step_bytes"], roofline["step_flops"] = sbytes, sflops
    if opt.full and not opt.no_roofline and rank == 0 and world == 1:
        # the GEMM launches of one captured step, replayed back to back from C++ with a HIP-event
        # pair around every launch (same arguments and buffers as the graph; see mesm_gemm_tape)
        istep = GraphedStep(model, crit, batch, args.dataset_name, warmup=1, instrument=True)
        istep.run()
        torch.cuda.synchronize()
        kn.gemm_tape_replay(1)  # warm
        prof = kn.gemm_tape_replay(opt.steps)
        if prof["launches"] > 0:
            avg_ms = prof["ms"] / prof["launches"]
            flops_per_launch = prof["flops"] / prof["launches"]
            achieved = flops_per_launch / (avg_ms * 1e-3) / 1e12
            lps = prof["launches"] / opt.steps
            traffic, tsrc = None, None
            tpath = os.path.join(ROOT, "profiles", "gemm_traffic.json")
            if os.path.exists(tpath):  # PMC FETCH_SIZE / WRITE_SIZE passes of this same command (tools/gpu_round.sh)
                with open(tpath) as f:
                    tj = json.load(f)
                if tj.get("hbm_bytes_per_step") and abs(tj.get("launch_calls_per_step", -1) - lps) < 0.5:
                    traffic = tj["hbm_bytes_per_step"] / lps
                    tsrc = "profiles/gemm_traffic.json (%s)" % tj.get("profile", "?")
                else:
                    tsrc = "profiles/gemm_traffic.json is stale (taken at %s launch calls/step, now %.0f)" \
                           % (tj.get("launch_calls_per_step"), lps)
            if os.path.exists(tpath) and tj.get("step_hbm_bytes_all_kernels"):
                # whole step, every kernel (same PMC passes): HBM-side bytes next to the algorithmic step_bytes
                roofline["step_traffic"] = tj["step_hbm_bytes_all_kernels"]
                roofline["step_traffic_source"] = "profiles/gemm_traffic.json (%s), FETCH_SIZE x 2 + WRITE_SIZE over every kernel" % tj.get("profile", "?")
            roofline.update({
                "kernel": "mesm_gemm_f32 family (gemm_wstage64_group / gemm_wstage64: v_mfma_f32_32x32x16_f16 x 3 over "
                          "operands split into two fp16 terms; gemm_wstage / gemm_lds64 / gemm_frag: v_mfma_f32_32x32x2_f32)"
                          if gemm_mode() == 2 else
                          "mesm_gemm_f32 family (gemm_wstage64_group / gemm_wstage64: v_mfma_f32_32x32x16_bf16 x 6 over "
                          "split operands; gemm_wstage / gemm_lds64 / gemm_frag: v_mfma_f32_32x32x2_f32)"
                          if gemm_mode() == 6 else
                          "mesm_gemm_f32 family (gemm_wstage / gemm_lds64 / gemm_frag / gemm_f32 kernels, v_mfma_f32_32x32x2_f32)",
                "achieved": achieved, "frac": achieved / PEAK_F32_MFMA_TFLOPS, "traffic": traffic,
                "traffic_source": tsrc, "launches_per_step": lps,
                "measured": "HIP event pair around the back-to-back GEMM launches of one captured step, "
                            "replayed %d x" % opt.steps,
                "avg_launch_us": avg_ms * 1e3, "flops_per_launch": flops_per_launch,
                "gemm_ms_per_step": prof["ms"] / opt.steps,
                "algorithmic_bytes_per_launch": prof.get("bytes", 0) / max(prof["launches"], 1),
                # the same with every side matrix the fused epilogues touch (residual, second output, aux, RMW read)
                "algorithmic_bytes_per_launch_with_side_operands": prof.get("bytes_with_sides", 0) / max(prof["launches"], 1)})
            if traffic:
                roofline["traffic_over_algorithmic"] = {
                    "operands_only": traffic / max(roofline["algorithmic_bytes_per_launch"], 1.0),
                    "with_side_operands": traffic / max(roofline["algorithmic_bytes_per_launch_with_side_operands"], 1.0)}

    # informational: the same steps with every batch arriving from HOST memory (PCIe-inclusive rate; never
    # `value`): the host batch goes through GraphedStep.load_batch (static inputs + rebuilt index plans)
    pcie = None
    if extras and not opt.eager and world == 1:
        for _ in range(3):
            gstep.load_batch(batch_cpu, redraw=True); gstep.run(redraw=False)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        for _ in range(opt.steps):
            gstep.load_batch(batch_cpu, redraw=True); gstep.run(redraw=False)
        torch.cuda.synchronize()
        pdt = (time.perf_counter() - t2) / opt.steps
        hb = sum(v.numel() * v.element_size() for v in batch_cpu.values() if torch.is_tensor(v))
        pcie = {"pairs_per_s": n_pairs / pdt, "ms_per_step": pdt * 1e3, "host_bytes_per_step": hb}

    # informational: a loader-like stream of batches (the reference's loaders emit a different number of pairs almost
    # every batch: an item is a video with ALL its queries, dataset/base.py:116-162; config batch_size = 12 videos).
    # Group sizes drawn from (roughly) the QVHighlights train histogram, every batch from HOST memory through
    # StepCache(pairs=16, group_caps=(5, 9)): pair axis padded to a multiple of 16 with the real count as a device scalar.
    loader = None
    if extras and not opt.eager and world == 1 and opt.workload == "C3a":
        try:
            import random
            from mesm_amd.graphed import StepCache
            rng = random.Random(5)
            sizes, probs = list(range(1, 10)), [0.18, 0.22, 0.20, 0.15, 0.10, 0.07, 0.04, 0.025, 0.015]
            cache = StepCache(model, crit, args.dataset_name, pad=(wl["Lv"], wl["Lw"]), pairs=16, group_caps=(5, 9))
            nb = 36
            stream_b = []
            for i in range(nb):
                groups = [rng.choices(sizes, probs)[0] for _ in range(12)]
                stream_b.append((groups, synthetic.make_batch(wl["dataset_name"], groups, wl["Lv"], wl["Lw"], wl["v_feat_dim"],
                                                              wl["t_feat_dim"], wl["vocab_size"] + 1, seed=1000 + i, ragged=True)))
            for _, hb in stream_b:  # first pass: every (pair bucket, group bucket) of the stream gets its graph
                cache.run(hb, redraw=True)
            torch.cuda.synchronize()
            c0, r0 = cache.captures, cache.replays
            t1 = time.perf_counter()
            for _, hb in stream_b:  # second pass, timed as a stream (host work of batch i + 1 overlaps replay i)
                cache.run(hb, redraw=True)
            torch.cuda.synchronize()
            tt = time.perf_counter() - t1
            r1 = cache.replays
            npairs = sum(sum(g) for g, _ in stream_b)
            # the same stream with the host half of every batch (padding, plans, targets) done by forked loader workers
            # (mesm_amd/loader.py; the reference hides its collate behind DataLoader(num_workers=8)): the training
            # process draws, uploads one arena, copies the pinned features and replays
            tw, wk = None, min(4, max(2, host_cores() // 4))
            try:
                from mesm_amd.loader import prepared_loader
                ld = prepared_loader([hb for _, hb in stream_b], cache.pipeline(keep_raw=False), num_workers=wk, pin_memory=False,
                                     ring=True)  # feature tensors through a shared page-locked ring, not the loader's queues
                for prep in ld:  # first pass: workers start, pinned buffers and staging get allocated
                    cache.run_prepared(prep)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for prep in ld:
                    cache.run_prepared(prep)
                torch.cuda.synchronize()
                tw = time.perf_counter() - t1
                del ld
            except Exception as e:
                log("loader-worker section skipped: %s: %s" % (type(e).__name__, e))
            # replay-only time of the same graphs on the same batches (no host work between replays)
            tr = None
            try:
                sel = []
                for _, hb in stream_b:
                    _, gs_ = cache.run(hb, redraw=False)
                    sel.append(gs_)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for gs_ in sel:
                    gs_.run(redraw=False)
                torch.cuda.synchronize()
                tr = time.perf_counter() - t1
            except Exception as e:
                log("replay-only section skipped: %s: %s" % (type(e).__name__, e))
            loader = {"batches": nb, "videos_per_batch": 12, "graphs_captured": c0,
                      "ms_per_step_with_loader_workers": None if tw is None else tw / nb * 1e3,
                      "loader_workers": wk, "pairs_per_s_with_loader_workers": None if tw is None else npairs / tw,
                      "ms_per_step_replay_only_same_graphs": None if tr is None else tr / nb * 1e3,
                      "first_pass_replayed_fraction": r0 / nb, "second_pass_replayed_fraction": (r1 - r0) / nb,
                      "ms_per_step_from_host": tt / nb * 1e3, "pairs_per_s": npairs / tt,
                      "mean_pairs_per_batch": npairs / nb,
                      "note": "second pass over the same 36 host batches, every graph warm; pair axis padded to a multiple "
                              "of 16 (real count = device scalar), group buckets (5, 9).  ms_per_step_from_host: all host "
                              "work in the training process; ms_per_step_replay_only_same_graphs: the same graphs replayed "
                              "without any host work (these batches average 41 pairs padded to 48 / 64 with groups of up "
                              "to 9 queries: a heavier step than the 32-pair headline); with_loader_workers: the host half "
                              "in forked DataLoader workers, feature tensors through a shared page-locked ring of host "
                              "slots (mesm_amd/loader.py PinnedRing): only descriptors cross the process boundary"}
            del cache
            # the same stream through the UNCHANGED caller: prepare_batch_input + train.py:64-72 with torch's optimizer, graph
            # replay behind the calls (model.autograph(pad=..., pairs=16): first visit of a bucket eager, second captures)
            try:
                from torch import nn
                from mesm_amd import batching as _bt
                model.autograph(True, pad=(wl["Lv"], wl["Lw"]), pairs=16)
                a0 = model._auto
                base_cap, base_rep, base_eag, base_hs = a0.captures, a0.replays, a0.eager, a0.host_side
                lopt = torch.optim.AdamW(model.parameters(), lr=0.0, weight_decay=1e-4)

                # (the batches page-locked, as a DataLoader(pin_memory=True) delivers them: train.py's loader does)
                pinned_b = [{k: (v.pin_memory() if torch.is_tensor(v) else
                                 ([{kk: vv.pin_memory() for kk, vv in d.items()} for d in v]
                                  if isinstance(v, list) and v and isinstance(v[0], dict) else v))
                             for k, v in hb.items()} for _, hb in stream_b]

                def epoch(keep_host):
                    # keep_host False: dataset/base.py:358-384's semantics exactly (what an unchanged train.py gets from the
                    # reference's own `dataset` package); True: this build's prepare_batch_input, which keeps the host copies
                    # of the small tensors it has in hand (batching.attach_host_side)
                    _bt._KEEP_HOST_SIDE = bool(keep_host)
                    for hb in pinned_b:
                        b_ = dict(hb)
                        b_ = _bt.prepare_batch_input(b_, dev, non_blocking=True)
                        out_ = model(**b_, dataset_name=args.dataset_name, is_training=True)
                        _, loss_ = crit(out_, b_, is_training=True)
                        lopt.zero_grad()
                        loss_.backward()
                        nn.utils.clip_grad_norm_(model.parameters(), 0.1)
                        lopt.step()
                    torch.cuda.synchronize()
                epoch(False); epoch(False)  # eager visits, then captures
                cap = a0.captures - base_cap
                r_before = a0.replays
                t1 = time.perf_counter(); epoch(False); t_plain = time.perf_counter() - t1
                rep_frac = (a0.replays - r_before) / nb
                epoch(True)
                t1 = time.perf_counter(); epoch(True); t_host = time.perf_counter() - t1
                loader["unchanged_caller"] = {
                    "ms_per_step": t_plain / nb * 1e3, "pairs_per_s": npairs / t_plain, "graphs_captured": cap,
                    "timed_pass_replayed_fraction": rep_frac,
                    "ms_per_step_with_this_builds_prepare_batch_input": t_host / nb * 1e3,
                    "note": "the same 36 host batches, page-locked like a DataLoader(pin_memory=True) delivers them, through "
                            "prepare_batch_input (asynchronous copies) and the reference's loop "
                            "body with torch's clip_grad_norm_ + AdamW (lr = 0); model.autograph(pad=(Lv, Lw), pairs=16)"}
            except Exception as e:
                log("unchanged-caller loader section skipped: %s: %s" % (type(e).__name__, e))
            finally:
                import mesm_amd.batching as _bt2
                _bt2._KEEP_HOST_SIDE = True
                model.autograph(False)
                model._auto.pad = model._auto.pairs = None
                model.zero_grad(set_to_none=True)
        except Exception as e:
            log("loader-like section skipped: %s: %s" % (type(e).__name__, e))

    # informational (NOT part of the metric, which is fwd + bwd): the optimizer tail of train.py:70-72 on
    # the flat buffers, global-norm clip + AdamW in two launches.  (Runs last: it changes the weights.)
    opt_tail_ms = None
    if extras:
        from mesm_amd.optim import FlatAdamW
        fo = FlatAdamW(model, lr=1e-4, weight_decay=1e-4)
        for _ in range(3):
            fo.step(grad_clip=0.1)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(20):
            fo.step(grad_clip=0.1)
        torch.cuda.synchronize()
        opt_tail_ms = (time.perf_counter() - t1) / 20 * 1e3

    # in-situ cost of each kernel family (tools/ablate.py): the captured step re-timed with that family's
    # launches turned into no-ops -- the attribution that adds up to the real step time (a kernel trace inflates
    # every short kernel by ~2 us).  Informational, after the timed region, default workload only.
    families = None
    if extras and not opt.eager and world == 1 and opt.workload == "C3a":
        try:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import ablate
            fc = ablate.family_costs(opt.workload, reps=10)
            families = {"gemm_ms": fc["gemm"], "attention_ms": fc["attn"], "layernorm_ms": fc["ln"],
                        "losses_ms": fc["loss"], "elementwise_ms": fc["elt"], "assembly_ms": fc["glue"],
                        "aten_and_launch_floor_ms": fc["floor"], "step_ms": fc["full_step"],
                        "method": "step time with the family's launches as no-ops (tools/ablate.py), dropout masks "
                                  "not redrawn"}
        except Exception as e:  # never let an informational section take the bench line down
            log("family attribution skipped: %s: %s" % (type(e).__name__, e))
    roofline["families"] = families
    if families is not None:
        # SURVEY 8d byte split of C3a (kernel-boundary traffic per step): attention cores 0.45 GB, LayerNorm 0.65 GB;
        # achieved fraction of the 8 TB/s HBM roofline of those two HBM-bound families, from their in-situ time
        def _hbm_frac(nbytes, ms):  # None rather than an exception: informational sections never take the line down
            return nbytes / (ms * 1e-3) / (PEAK_HBM_TBS * 1e12) if isinstance(ms, (int, float)) and ms > 0 else None
        roofline["attention_hbm_frac"] = _hbm_frac(0.45e9, families.get("attention_ms"))
        roofline["layernorm_hbm_frac"] = _hbm_frac(0.65e9, families.get("layernorm_ms"))

    # The same step in the other GEMM arithmetics and with the forward's atomically summed products off, each in a child
    # process (the switches are read once at load): `exact_f32` = every product on v_mfma_f32_32x32x2_f32
    # (MESM_GEMM_BF16X=0; `exact_f32_ms` beside the headline so a reader sees both); `bf16x6` = round 4's split;
    # `deterministic_ms_per_step` = MESM_GEMM_FWD_ATOMICS=0 (K-split forward products off: bit-reproducible loss).
    if extras and not opt.eager and world == 1 and opt.workload == "C3a" and "MESM_GEMM_BF16X" not in os.environ:
        def child(**env):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(opt.steps), "--warmup",
                                    str(opt.warmup), "--cpu-steps", "0", "--no-extras", "--full"],
                                   env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
                lj = json.loads(r.stdout.strip().splitlines()[-1])
                return {"ms_per_step": lj["ms_per_step"], "gemm_tflops": lj["roofline"]["achieved"],
                        "gemm_ms_per_step": lj["roofline"].get("gemm_ms_per_step"), "dtype": lj["dtype"]}
            except Exception as e:
                return {"error": "%s: %s" % (type(e).__name__, e)}
        ex = child(MESM_GEMM_BF16X="0")
        roofline["exact_f32"] = ex
        roofline["exact_f32_ms"] = ex.get("ms_per_step")
        roofline["bf16x6"] = child(MESM_GEMM_BF16X="6")
        if "MESM_GEMM_FWD_ATOMICS" not in os.environ:
            roofline["deterministic_ms_per_step"] = child(MESM_GEMM_FWD_ATOMICS="0").get("ms_per_step")
    mode = gemm_mode()
    if roofline.get("achieved") and mode in (2, 6):
        # what the matrix pipes see: `per` half-precision products per algorithmic f32 product on the launches that take
        # the split path (an upper bound: it prices EVERY GEMM flop of the step that way, the small 32 x 32-tile launches
        # still run v_mfma_f32_32x32x2_f32).  The two honest ceilings side by side: `frac` = algorithmic f32
        # flops / the f32 matrix peak (what an exact-f32 kernel could reach: continuity with earlier rounds); `frac_issue` =
        # the same flops / the ceiling of a kernel that issues `per` 16-bit products per f32 flop, 2.5 PF / per
        per = 3.0 if mode == 2 else 6.0
        roofline["half_mfma_issue"] = {"products_per_flop": per, "achieved_upper": per * roofline["achieved"],
                                       "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s",
                                       "frac_upper": per * roofline["achieved"] / PEAK_BF16_MFMA_TFLOPS}
        roofline["issue_peak"] = PEAK_BF16_MFMA_TFLOPS / per
        roofline["frac_issue"] = roofline["achieved"] / (PEAK_BF16_MFMA_TFLOPS / per)
        roofline["arithmetic"] = (
            "operands scaled by a wave-owned power of two and split into hi = f16_rne(x), lo = f16_rne(x - hi) (22-24 "
            "significand bits), products lo*hi, hi*lo, hi*hi on v_mfma_f32_32x32x16_f16, f32 accumulate, accumulators rescaled "
            "when a stage leaves the scale's band" if mode == 2 else
            "operands split exactly into hi + mid + lo bf16 (x = hi + mid + lo), products lo*hi, hi*lo, mid*mid, mid*hi, "
            "hi*mid, hi*hi on v_mfma_f32_32x32x16_bf16, f32 accumulate") + (
            "; `achieved` / `frac` stay ALGORITHMIC f32 flops against the f32 MFMA peak (157.3 TF)")

    # run-to-run spread of the replayed step: two replays of one batch with the same draws and dropout masks off (the
    # float atomics of split-K products order by arrival); gradient difference / gradient norm, loss difference
    spread = None
    if extras and not opt.eager and world == 1 and opt.workload == "C3a":
        try:
            saved_p = {}
            for m_ in model.modules():
                if hasattr(m_, "p") and isinstance(getattr(m_, "p"), float):
                    saved_p[m_] = m_.p
                    m_.p = 0.0
            rstep = GraphedStep(model, crit, batch, args.dataset_name, warmup=1)
            rstep.run(redraw=False); torch.cuda.synchronize()
            g1, l1 = model.gradbuf().flat.clone(), float(rstep.total)
            worst, lworst = 0.0, 0.0
            for _ in range(4):
                rstep.run(redraw=False); torch.cuda.synchronize()
                worst = max(worst, float((model.gradbuf().flat - g1).norm() / g1.norm()))
                lworst = max(lworst, abs(float(rstep.total) - l1))
            spread = {"grad_rel_l2_max_of_4_replays": worst, "loss_abs_max": lworst,
                      "fwd_atomics": os.environ.get("MESM_GEMM_FWD_ATOMICS", "1")}
            del rstep
        except Exception as e:
            spread = {"error": "%s: %s" % (type(e).__name__, e)}
        finally:
            for m_, p_ in saved_p.items():
                m_.p = p_
        roofline["run_to_run_grad_spread"] = spread

    # the other BASELINE.json configs that fit one GPU, one graph each, 10 steps (child processes; not the metric)
    others = None
    if extras and not opt.eager and world == 1 and opt.workload == "C3a" and not opt.no_roofline:
        others = {}
        for w in ("C2", "C3b", "C5"):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", w, "--steps", "10", "--warmup", "3",
                                    "--cpu-steps", "0", "--no-extras", "--no-roofline"], capture_output=True, text=True, timeout=300)
                lj = json.loads(r.stdout.strip().splitlines()[-1])
                others[w] = {"ms_per_step": lj["ms_per_step"], "pairs_per_s": lj["value"],
                             "step_hbm_frac": lj["roofline"]["step_hbm_frac"], "step_mfma_frac": lj["roofline"]["step_mfma_frac"],
                             "workload": lj["config"]["workload"]}
            except Exception as e:
                others[w] = {"error": "%s: %s" % (type(e).__name__, e)}

    cpu_baseline = None
    if opt.full and rank == 0 and world == 1 and opt.cpu_steps > 0:
        from oracle import mesm_oracle as O
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        cfg = dict(vars(args))
        neg, masked = synthetic.host_draws(batch_cpu, seed=0)
        ncores = min(host_cores(), 64)
        torch.set_num_threads(ncores)
        log("cpu baseline on %d threads" % ncores)
        # TRAIN mode like the GPU leg: every nn.Dropout of the reference active (CPU bernoulli masks)
        O.DROPOUT = (float(args.dropout), float(args.input_dropout))
        try:
            for _ in range(2):
                O.train_step(sd, cfg, batch_cpu, neg, masked)  # warm-up
            log("cpu warm-up done")
            ts = []
            for _ in range(opt.cpu_steps):
                c0 = time.perf_counter()
                O.train_step(sd, cfg, batch_cpu, neg, masked)
                ts.append(time.perf_counter() - c0)
        finally:
            O.DROPOUT = None
        med = sorted(ts)[len(ts) // 2]
        cpu_baseline = {"value": n_pairs / med, "unit": "pairs/s", "cores": ncores, "kind": "port",
                        "sample": "median of %d fwd+bwd steps (after 2 warm-up) of %s (%d pairs each), train mode "
                                  "(dropout on), torch-CPU fp32" % (opt.cpu_steps, opt.workload, n_pairs)}

    if rank == 0:
        line = {
            "metric": "clip-query pairs/sec (fwd+bwd)", "value": n_pairs * world / t_step,
            "unit": "pairs/s", "n_gpus": world, "steps": opt.steps, "warmup": opt.warmup,
            "ms_per_step": t_step * 1e3, "host_ms_per_step": host_ms, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": dtype_name(), "data": "synthetic",
            "config": {"workload": "%s: %s, %d pairs/GPU (%d groups), Lv=%d, Lw=%d, "
                                   "Dv=%d, Dt=%d, C=%d, 10 moment queries, train mode (dropout on)"
                                   % (opt.workload, {"qvhighlights": "QVHighlights C+SF", "charades": "Charades-STA",
                                                     "tacos": "TACoS C3D"}.get(wl["dataset_name"], wl["dataset_name"]),
                                      n_pairs, len(wl["groups"]), wl["Lv"], wl["Lw"],
                                      wl["v_feat_dim"], wl["t_feat_dim"], wl["vocab_size"] + 1),
                       "global_pairs": n_pairs * world, "parallelism": "dp%d" % world,
                       "launch": "eager" if opt.eager else "hip-graph", "ddp": ddp_mode, "ddp_diag": ddp_diag,
                       "host_draws": draws_mode(), "full": opt.full,
                       "settled_not_in_metric": settled,
                       "eager_ms_per_step_not_in_metric": eager_ms,
                       # train.py:64-72 verbatim with the optimizer train.py itself gets from build_optimizer (line 115; all three
                       # factories of lines 17-18 from this build); the same body with torch.optim.AdamW: `..._not_in_metric.ms_per_step`
                       "unchanged_caller_ms_per_step": (unchanged.get("loop_body_unchanged_with_all_three_factories_from_this_build_ms")
                                                        if unchanged else None),
                       "unchanged_caller_with_torch_adamw_ms_per_step": unchanged.get("ms_per_step") if unchanged else None,
                       "unchanged_caller_not_in_metric": unchanged,
                       "other_workloads_not_in_metric": others,
                       "optimizer_tail_ms_not_in_metric": opt_tail_ms,
                       "pcie_inclusive_not_in_metric": pcie,
                       "loader_like_epoch_not_in_metric": loader},
            "roofline": roofline, "cpu_baseline": cpu_baseline,
        }
        try:  # whatever native libraries left in C stdio buffers (RCCL's version banner) goes out BEFORE the result line
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(line), flush=True)
    if world > 1:
        # leave together and without tearing the communicator down: destroying a RCCL process group next to live
        # HIP graphs has aborted the interpreter on this stack (tests/ddp_capture_worker.py leaves the same way),
        # and a crash after the result line would still fail the run
        sys.stdout.flush()
        sys.stderr.flush()
        dist.barrier()
        torch.cuda.synchronize()
        os._exit(0)


if __name__ == "__main__":
    main()
