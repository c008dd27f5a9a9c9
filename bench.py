#!/usr/bin/env python3
"""bench.py -- images/sec of the INT8 hot path on MI355X.

Workload (BASELINE.json configs[3]/[4]): AlexNet INT8, 224x224, global batch
1000, random-init weights + synthetic inputs (the reference's checkpoints and
CIFAR-10 are not available offline).  One "step" = the reference notebook's
timed cell (sample/notebooks/AlexNet_cifar10_resize224.ipynb:212-218) for one
batch: model(x) [quantize -> 5 conv / 3 fc INT8 layers with u8 relu / max-pool
-> dequantize], logits to the host, argmax, compare with the labels.  Inputs
are resident in HBM before the timed region (the notebook builds its tensors
beforehand, :112-114).

    python bench.py --gpus 1 --steps 20 --warmup 3
    python bench.py --gpus 8 --steps 20 --warmup 3        (starts the 8 ranks itself, as a child torch.distributed.run)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \\
        --master-port P bench.py --gpus N --steps K --warmup W

N > 1: one process per GPU; the 1000 images shard contiguously over the ranks
(strong scaling, as BASELINE.json configs[4] names it), each rank runs the full
network on its shard and one RCCL all-gather collects the logits.
Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times --steps steps and prints the headline
(images/sec, ms_per_step).  --full adds everything else this script measures or
checks: HIP events sampled in the timed region, the other step discipline, the
per-kernel breakdown and roofline, the PCIe-inclusive rate, the FP32 path, the
CPU oracle baseline and logit parity against it.

    python bench.py --gpus 1 --steps 20 --warmup 3 --full
    python bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs DIR

--dump-outputs DIR writes what the last timed step returned (rank 0's gathered
logits, float32, and the host top-1 classes) as DIR/logits.npy and
DIR/top1_class.npy; weights and inputs are seeded, so two builds can be
compared output for output.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

INT8_DENSE_PEAK_TOPS = 5000.0  # MI355X dense int8 MFMA: 2x the ~2.5 PF bf16 rate (MI355X_MICROARCH.md, Matrix cores)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1000, help="global batch (images per step over all GPUs)")
    ap.add_argument("--network", default="alexnet")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU oracle baseline and parity")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="target CPU time of the oracle baseline sample")
    ap.add_argument("--force-dist", action="store_true", help="take the torch.distributed path even with one rank")
    ap.add_argument("--weak", action="store_true",
                    help="weak scaling: --batch images PER GPU (global batch = batch x GPUs); default is the strong "
                         "scaling BASELINE.json configs[4] names (global batch fixed, sharded)")
    ap.add_argument("--graph", choices=("auto", "on", "off"), default="auto",
                    help="replay the forward as one HIP graph (int8inferenceengine_amd/graph.py); auto: when this rank's "
                         "shard is at most 256 images, where the eager forward is launch-bound")
    ap.add_argument("--sync-steps", action="store_true",
                    help="read every batch's logits before launching the next batch (no software pipeline)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline figure (untimed passes, per-kernel "
                         "breakdown, roofline, PCIe rate, FP32 path, CPU baseline, parity); off: headline only")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the last timed step's logits and top-1 classes to DIR/<name>.npy (rank 0)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        if world == 1 and args.gpus > 1 and "RANK" not in os.environ:
            # `python bench.py --gpus N` as typed: one process per GPU is the model, so start the ranks as a CHILD
            # (torch.distributed.run) and relay its exit code.  Nothing has touched torch or HIP in this process yet, and it
            # never will: the child does the work (no exec: a process image is never replaced here).
            import socket
            import subprocess

            with socket.socket() as s:  # a free rendezvous port on the loopback
                s.bind(("127.0.0.1", 0))
                port = s.getsockname()[1]
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
                   "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
            env = dict(os.environ, MASTER_ADDR="127.0.0.1")
            env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # (dmabuf IPC: RCCL between processes needs it on this host driver)
            sys.exit(subprocess.run(cmd, env=env).returncode)  # rank 0's JSON line goes straight to our stdout
        args.gpus = world
    use_dist = world > 1 or args.force_dist

    import numpy as np

    import torch  # first: libi8ie_hip.so must bind to the HIP runtime torch already loaded
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx
    import i8ie
    from int8inferenceengine_amd import sharding
    from int8inferenceengine_amd import workloads as wl

    if not torch.cuda.is_available():
        sys.exit("bench.py: no GPU visible (the INT8 path has no CPU fallback)")
    # Rehearsal of the N > 1 control flow on a box with one GPU (RCCL refuses two ranks on one device): every
    # rank uses device 0 and the collectives run over gloo on host copies.  Not a measurement.
    rehearse = bool(os.environ.get("I8IE_BENCH_REHEARSE"))
    if rehearse:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    if use_dist:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group("gloo" if rehearse else "nccl", rank=rank, world_size=world)  # "nccl" is RCCL on ROCm
        # run our kernels on torch's current stream so the collective is stream-ordered behind them; a stream of
        # its own rather than the legacy default stream (which cannot be captured into a HIP graph and serialises
        # with every blocking stream)
        torch.cuda.set_stream(torch.cuda.Stream())
        cx.use_stream(torch.cuda.current_stream().cuda_stream, local_rank)
    else:
        cx.set_device(local_rank)

    name = args.network
    n_total = args.batch * world if args.weak else args.batch
    start, stop = sharding.shard_bounds(n_total, rank, world)

    # ---- model: the reference workflow, prepare -> one FP32 batch -> convert (identical on every rank)
    sd = wl.synthetic_state_dict(name, seed=42)
    net = wl.calibrated(name, sd)
    qparams = {a: getattr(net, a).output_qparams() for a in wl.layer_names(name)}

    # ---- inputs + FP32-teacher labels (centred argmax)
    x_all = wl.synthetic_input(name, n_total, seed=1234)
    x_loc = np.ascontiguousarray(x_all[start:stop])
    fp32_net = wl.build(name)
    fp32_net.load(sd)
    centre = fp32_net(i8ie.tensor(wl.synthetic_input(name, 64, seed=4321))).numpy().mean(0)
    x_fp = i8ie.tensor(x_loc).prefetch()
    cx.synchronize()
    t_fp0 = time.perf_counter()
    fp_logits = fp32_net(x_fp).numpy()
    fp32_ms = (time.perf_counter() - t_fp0) * 1e3  # the engine's FP32 path, one pass
    lab_loc = sharding.centred_argmax(fp_logits, centre)
    del fp32_net, x_fp
    cx.trim()
    def gather(t):  # [rows_local, C] on the GPU -> [n_total, C] on every rank
        return sharding.gather_rows(t.cpu() if rehearse else t, n_total)

    if use_dist:
        lab_all = gather(torch.from_numpy(lab_loc.astype(np.float32)[:, None]).cuda())
        lab_all = lab_all.cpu().numpy()[:, 0].astype(np.int64)
    else:
        lab_all = lab_loc

    t_h2d0 = time.perf_counter()
    x_dev = i8ie.tensor(x_loc).prefetch()  # resident in HBM before the timed region
    cx.synchronize()
    h2d_ms = (time.perf_counter() - t_h2d0) * 1e3
    # N > 1: the package's runner owns the stage buffers, the side stream, the all-gather and rank 0's read-back
    use_graph = args.graph == "on" or (args.graph == "auto" and (stop - start) <= 256)
    graphed = None
    if use_graph:
        from int8inferenceengine_amd.graph import GraphedForward
        graphed = GraphedForward(net, x_dev)  # one eager forward, then the same launches recorded as a HIP graph
    runner = sharding.ShardedRunner(net, n_total, 10, rank, world, host_copies=rehearse) if use_dist else None
    mode = {"eager": False}

    state = {"correct": 0, "logits": None}

    def forward(x):
        return graphed() if (graphed is not None and not mode["eager"]) else net(x)

    if runner is not None:
        runner.forward = forward

    def launch():
        """Queue one batch: quantize -> INT8 layers -> dequantize -> (gather) -> logits towards the host.
        Nothing here waits for the GPU."""
        if not use_dist:
            return forward(x_dev).numpy_async()
        return runner.submit(x_dev)

    def consume(h):
        """Wait for one batch's logits, top-1 on the host (the reference's argmax + compare)."""
        logits = runner.result(h) if use_dist else h.result()
        if rank != 0:
            return
        pred = sharding.centred_argmax(logits, centre)
        state["correct"] = int((pred == lab_all).sum())
        state["logits"] = logits

    def run_steps(k, pipelined):
        """k batches.  pipelined: batch i+1 is launched before batch i's logits are awaited (depth 2), so the
        read-back, gather latency and host argmax of one batch hide behind the kernels of the next."""
        pending = None
        for _ in range(k):
            h = launch()
            if not pipelined:
                consume(h)
                continue
            if pending is not None:
                consume(pending[0])
            pending = (h,)
        if pending is not None:
            consume(pending[0])

    pipelined = not args.sync_steps

    def barrier():
        if use_dist:
            dist.barrier()

    # untimed pre-warm: a second of steps so that clocks, allocator and caches are in steady state
    # before the contract's W warm-up steps (a fresh box measures its first ~20 steps 3-5 % slow)
    # (same count on every rank -- the steps contain a collective)
    prewarm = 0 if os.environ.get("I8IE_BENCH_NO_PREWARM") else max(10, min(150, int(0.25 / (sharding.max_shard(n_total, world) * 2.1e-6 + 1.5e-4))))
    run_steps(prewarm, pipelined)
    run_steps(args.warmup, pipelined)
    barrier()
    torch.cuda.synchronize()
    sample_events = args.full and rank == 0 and not os.environ.get("I8IE_BENCH_NO_EVENTS") and graphed is None
    if sample_events:
        # HIP events around contraction-kernel launches, on the stream the kernels run on.  Every event
        # packet costs a few microseconds of stream time (bracketing all 9 contraction launches of a step:
        # ~5 % of the step), so the timed region brackets every 5th contraction launch -- coprime with the
        # launches per step, so every kernel and shape is sampled; the untimed pass below brackets all.
        cx.profile_start(mfma_only=True, stride=5)
    t0 = time.perf_counter()
    run_steps(args.steps, pipelined)
    torch.cuda.synchronize()
    barrier()
    elapsed = time.perf_counter() - t0
    prof = cx.profile_stop() if sample_events else {}
    # the last timed step's logits (rank 0), kept apart from the untimed passes below
    last_logits = None if state["logits"] is None else np.array(state["logits"], np.float32)
    if args.full:
        # untimed: the same batches with the other step discipline, for the record
        barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        run_steps(args.steps, not pipelined)
        torch.cuda.synchronize()
        barrier()
        other_ms = (time.perf_counter() - t1) / args.steps * 1e3
        mode["eager"] = True  # the per-kernel breakdown needs individual launches: graph replays are not bracketed
        if rank == 0:  # untimed pass with every launch bracketed: the per-kernel breakdown
            cx.profile_start(mfma_only=False)
            run_steps(args.steps, pipelined)
            full = cx.profile_stop()
        else:
            run_steps(args.steps, pipelined)  # keep the collectives matched
        mode["eager"] = False
    # ---- untimed: PCIe-inclusive rate.  The FP32 batch starts in pinned host memory, its upload runs on the
    # transfer stream beside the kernels of the batch before (two pinned buffers, two device blocks).
    pcie = None
    if args.full and world == 1 and not use_dist:
        pin = [i8ie.pinned_empty(x_loc.shape) for _ in range(2)]
        for b in pin:
            b[...] = x_loc
        k_pcie = max(4, min(args.steps, 10))

        def pcie_steps(k):
            pending = None
            for i in range(k):
                h = net(i8ie.tensor(pin[i & 1])).numpy_async()
                if pending is not None:
                    consume(pending)
                pending = h
            consume(pending)

        pcie_steps(2)
        cx.synchronize()
        tp0 = time.perf_counter()
        pcie_steps(k_pcie)
        cx.synchronize()
        pcie_ms = (time.perf_counter() - tp0) / k_pcie * 1e3
        pcie = {"ms_per_step": round(pcie_ms, 3), "images_per_sec": round(n_total / (pcie_ms * 1e-3), 1),
                "gbytes_per_sec_h2d": round(x_loc.nbytes / (pcie_ms * 1e-3) / 1e9, 1), "steps": k_pcie,
                "how": "FP32 batch in pinned host memory, async upload on the transfer stream overlapped with the previous batch's kernels"}
        del pin
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if rehearse else "cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if rank != 0:
        if use_dist:
            dist.barrier()
            dist.destroy_process_group()
        return

    ms_per_step = elapsed / args.steps * 1e3
    value = n_total * args.steps / elapsed

    if args.dump_outputs:  # what a caller of the timed path receives from its last step
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "logits.npy"), last_logits)
        np.save(os.path.join(args.dump_outputs, "top1_class.npy"),
                sharding.centred_argmax(last_logits, centre).astype(np.float32))

    if args.full:
        # ---- roofline of the dominant kernel (by device time) --------------------------------------
        def table(raw):
            return {k: {"launches": int(v[0]), "ms": v[1], "ops": v[2], "bytes": v[3]} for k, v in raw.items()}

        def by_kernel(shapes):  # entries are "kernel|shape": group by kernel
            out = {}
            for k, v in shapes.items():
                e = out.setdefault(k.split("|")[0], {"launches": 0, "ms": 0.0, "ops": 0.0, "bytes": 0.0})
                for f in e:
                    e[f] += v[f]
            return out

        per_shape = table(full)                 # untimed pass: every launch of every kernel bracketed
        kernels = by_kernel(per_shape)
        timed = by_kernel(table(prof)) if prof else kernels  # timed region: sampled contraction launches
        mfma = {k: v for k, v in kernels.items() if v["ops"] > 0}
        dom = max(mfma, key=lambda k: mfma[k]["ms"])
        d = timed.get(dom, mfma[dom])
        achieved = d["ops"] / (d["ms"] * 1e-3) / 1e12
        # HBM bytes per launch of the dominant kernel: rocprofv3 PMC passes are collected offline (counter collection
        # serialises every dispatch) and committed with the commit they were taken at; used only when they describe
        # this kernel at this workload, otherwise null
        traffic, traffic_meta = None, None
        for cand in ("r04_traffic.json", "r03_traffic.json", "r02_traffic.json", "r01_traffic.json"):
            try:
                tj = json.load(open(os.path.join(ROOT, "profiles", cand)))
                if tj.get("kernel") == dom and n_total == 1000 and world == 1 and name == "alexnet":
                    traffic = tj["hbm_bytes_per_launch"]
                    traffic_meta = {"file": "profiles/" + cand, "source": tj.get("source"), "collected_at_commit": tj.get("commit"),
                                    "algorithmic_bytes_per_launch": tj.get("algorithmic_bytes_per_launch")}
                    break
            except (OSError, ValueError, KeyError):
                pass
        roofline = {
            "bound": "mfma", "kernel": dom, "achieved": round(achieved, 2), "peak": INT8_DENSE_PEAK_TOPS,
            "unit": "TOP/s", "frac": round(achieved / INT8_DENSE_PEAK_TOPS, 4), "traffic": traffic,
            "traffic_provenance": traffic_meta,
            "ops_per_launch": d["ops"] / d["launches"], "avg_launch_ms": round(d["ms"] / d["launches"], 4),
            "launches_per_step": mfma[dom]["launches"] / args.steps,
            "launches_timed": d["launches"], "timed_in": "the timed region (every 5th contraction launch bracketed)" if prof else "untimed pass",
            "avg_launch_ms_untimed_pass_all_launches": round(mfma[dom]["ms"] / mfma[dom]["launches"], 4),
        }
        # NOT measured by this run: constants from committed profiles, kept apart from the measured fields above
        static_context = {
            "note": "constants from earlier measurements on MI355X, for reading `roofline`; nothing here is measured by this run",
            "register_only_int8_mfma_tops": {"random_operands": 3400.0, "constant_operands": 4860.0,
                                             "source": "profiles/r01h_mfma_peak_and_power.txt (tools/mfma_peak.hip)"},
            "in_kernel_clock_mhz_contraction_kernels_random_operands": {"range": [1880, 2174], "median": 2061, "nominal": 2400,
                                                                        "source": "profiles/r02_inkernel_clock.txt (s_memtime / s_memrealtime stamps, csrc/i8ie_pp.hip diagnostic builds)"},
        }
        total_dev_ms = sum(v["ms"] for v in kernels.values())
        breakdown = {k: round(v["ms"] / args.steps, 4) for k, v in sorted(kernels.items(), key=lambda kv: -kv[1]["ms"])}
        per_layer = {k: {"ms": round(v["ms"] / args.steps, 4),
                         "tops": round(v["ops"] / (v["ms"] * 1e-3) / 1e12, 1) if v["ops"] else None,
                         "gbps": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1)}
                     for k, v in sorted(per_shape.items(), key=lambda kv: -kv[1]["ms"])}
        macs = wl.macs_per_image(name)
        whole = {"int8_tops_whole_step": round(value * macs * 2 / 1e12, 2),
                 "frac_of_int8_peak_whole_step": round(value * macs * 2 / 1e12 / INT8_DENSE_PEAK_TOPS, 4),
                 "device_ms_per_step": round(total_dev_ms / args.steps, 3)}

        # ---- CPU baseline: the oracle (C restatement of the reference algorithm) on the host cores --
        cpu = None
        parity = None
        if world == 1 and not args.no_cpu_baseline:
            import orc
            import pipeline

            # a 1-GPU box gives this job a 16-CPU share; libgomp is already initialised (torch), so set it by call
            orc.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", min(len(os.sched_getaffinity(0)), 16))))

            entry = wl.NETWORKS[name]
            qlayers = pipeline.quantize_layers(entry, sd)
            probe = min(8, n_total)
            tp = time.perf_counter()
            pipeline.forward(entry, x_all[:probe], qlayers, qparams)
            rate = probe / (time.perf_counter() - tp)
            sample = int(max(probe, min(n_total, rate * args.cpu_seconds)))
            passes = 0
            tp = time.perf_counter()
            while True:  # whole passes over the sample until ~cpu_seconds of CPU work (at most 8 passes)
                ref_logits = pipeline.forward(entry, x_all[:sample], qlayers, qparams)
                passes += 1
                cpu_s = time.perf_counter() - tp
                if passes >= 8 or cpu_s * (passes + 1) / passes > args.cpu_seconds:
                    break
            cpu = {"value": round(sample * passes / cpu_s, 2), "unit": "images/sec", "cores": orc.num_threads(), "kind": "port",
                   "sample": "%d pass(es) over %d of the %d images of the same batch, full network, %.1f s"
                             % (passes, sample, n_total, cpu_s),
                   "host": open("/proc/cpuinfo").read().split("model name")[1].split("\n")[0].strip(": \t")}
            # ---- the same baseline with the reference's own GEMM provider (Intel MKL cblas_gemm_s8u8s32) when its
            # runtime is on this host and exact here; in a clean process, on a bounded sample (oracle/cpu_baseline_worker.py)
            try:
                import subprocess
                import tempfile

                k_mkl = int(min(sample, 400))
                blob = {"entry_json": np.asarray(json.dumps([entry[0], entry[1], list(entry[2])])), "x": x_all[:k_mkl],
                        "ref_logits": ref_logits[:k_mkl]}
                for a, (qw_, qb_, sw_) in qlayers.items():
                    blob[a + "__qw"], blob[a + "__qb"], blob[a + "__sw"] = qw_, qb_, np.float32(sw_)
                    blob[a + "__qp"] = np.asarray([qparams[a][0], qparams[a][1]], np.float64)
                with tempfile.TemporaryDirectory() as td:
                    np.savez(os.path.join(td, "in.npz"), **blob)
                    env = dict(os.environ, MKL_THREADING_LAYER="GNU", OMP_NUM_THREADS=str(orc.num_threads()))
                    subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "cpu_baseline_worker.py"),
                                    os.path.join(td, "in.npz"), os.path.join(td, "out.json"), str(orc.num_threads()),
                                    str(min(8.0, args.cpu_seconds * 0.5))], check=True, timeout=180, env=env,
                                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                    mk = json.load(open(os.path.join(td, "out.json")))
            except Exception as e:  # the MKL leg is optional: never let it take the bench line down
                mk = {"provider": None, "error": type(e).__name__}
            cpu["gemm"] = "own AVX-512/AVX2 loop (oracle/i8ie_oracle.c)"
            cpu["with_reference_gemm_provider"] = mk
            if mk.get("provider") and mk.get("logits_bit_exact_vs_own_kernel") and mk["images_per_sec"] > cpu["value"]:
                # the reference calls exactly this routine; where it is also the faster one (Intel hosts) it is the
                # headline baseline.  (On the AMD hosts of the MI355X boxes MKL 2021.4 takes a generic path ~10x slower
                # than the oracle's own VNNI loop, so the own loop stays the stronger, reported baseline there.)
                cpu["value_own_gemm"] = cpu["value"]
                cpu["value"] = mk["images_per_sec"]
                cpu["gemm"] = "Intel MKL cblas_gemm_s8u8s32, the reference's provider (%s)" % mk["provider"][:70]
                cpu["sample"] = "%d pass(es) over %d of the %d images of the same batch, full network, %.1f s" % (
                    mk["passes"], mk["images"], n_total, mk["seconds"])
            got = state["logits"][:sample]
            t_gpu = float((sharding.centred_argmax(got, centre) == lab_all[:sample]).mean())
            t_cpu = float((sharding.centred_argmax(ref_logits, centre) == lab_all[:sample]).mean())
            parity = {"logits_bit_exact_vs_oracle": bool(np.array_equal(got.view(np.uint32), ref_logits.view(np.uint32))),
                      "top1_vs_fp32_teacher_gpu": round(t_gpu, 4), "top1_vs_fp32_teacher_cpu_oracle": round(t_cpu, 4),
                      "top1_delta": round(abs(t_gpu - t_cpu), 6), "images_compared": sample}

    out = {
        "metric": "images/sec %s-INT8 %dx%d bs=%d" % (("AlexNet" if name == "alexnet" else name,) + wl.NETWORKS[name][2][1:] + (n_total,)),
        "value": round(value, 1), "unit": "images/sec",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True, "scaling": "weak" if args.weak else "strong", "vs_baseline": None, "dtype": "int8", "data": "synthetic",
        "config": {"workload": "%s INT8 forward + top-1, %dx%dx%d input, global batch %d sharded over %d GPU(s)"
                   % ((name,) + wl.NETWORKS[name][2] + (n_total, world)),
                   "global_batch": n_total, "per_gpu_batch": stop - start, "parallelism": "batch-shard x%d + logits all-gather" % world},
    }
    if args.full:
        out.update({"roofline": roofline, "cpu_baseline": cpu, "parity": parity, "whole_step": whole, "static_context": static_context,
                    "kernel_ms_per_step": breakdown, "per_launch_shape": per_layer})
    out.update({
        "top1_vs_fp32_teacher": round(state["correct"] / n_total, 4),
        "prewarm_steps_untimed": prewarm,
        **({"REHEARSAL": "all ranks on one GPU, gloo collectives on host copies: control flow only, not a measurement"}
           if rehearse else {}),
        "launch_mode": ("one HIP graph replay per batch (%d kernel nodes of %d nodes; int8inferenceengine_amd/graph.py)" % (graphed.kernel_nodes, graphed.nodes)
                        if graphed is not None else "eager launches"),
        "step_discipline": ("depth-2 software pipeline: batch i+1 is launched before batch i's logits are awaited"
                            if pipelined else "synchronous: logits of batch i read before batch i+1 is launched"),
    })
    if args.full:
        out.update({
            ("ms_per_step_synchronous" if pipelined else "ms_per_step_pipelined"): round(other_ms, 4),
            ("value_synchronous" if pipelined else "value_pipelined"): round(n_total / (other_ms * 1e-3), 1),
            "h2d_ms_fp32_input_pageable_blocking": round(h2d_ms, 2),
            "pcie_inclusive": pcie,
            "fp32_engine_path": {"images_per_sec": round((stop - start) / (fp32_ms * 1e-3), 1), "ms": round(fp32_ms, 1),
                                 "how": "one forward of this rank's shard through the FP32 layers (pre-convert path: "
                                        "Conv2d / Linear on v_mfma_f32_32x32x2_f32), input resident, logits read back"},
        })
    print(json.dumps(out), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
