"""The fused multi-head attention against the composition it replaces.

    python tools/bench_mha.py [--iters 20] [--rounds 5] [--warmup 5] [--net-steps 20] [--out profiles/r17_bench_mha.json]

Per shape (t tokens, c = H * d channels) and at 1000 and 125 images: ONE i8ie_attention_u8 launch over all heads against the
existing entries driven per head through pointer offsets -- i8ie_bmm_u8 (scores), i8ie_softmax_u8, i8ie_bmm_u8 (apply), 3 * H
launches with the [images, t, t] scores and probabilities in device memory -- in the same session on the same buffers.  Timing
is the library's own per-launch HIP-event bracket (i8ie_profile_start / _stop): `warmup` calls unprofiled, then `rounds` rounds
of `iters` profiled calls; a round's figure is its mean per call and the reported one the median over rounds.  Run-to-run spread
of these figures is about +-3 %.  The aim is fused <= composition (ratio <= 1); every row records the ratio and met or MISSED.
Before the timing the fused result of the first images is asserted against tests/mha_ref.py (the numpy definition) and the whole
fused result against the composition's.  Then the step of workloads' botnet_cifar (the network of examples/botnet_cifar10.py)
through the Python surface with the share its attention launches take of the kernel time."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
BATCHES = [1000, 125]
SHAPES = [("cifar_t64_c128_h1", 64, 128, 1), ("t64_c256_h4", 64, 256, 4), ("t256_c256_h4", 256, 256, 4), ("t1024_c128_h2", 1024, 128, 2)]
CHECKED_IMAGES = 2
f32 = np.float32


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("total_ops", C.c_double),
                ("total_bytes", C.c_double)]


def kernels(args):
    import attention_ref as ar
    import mha_ref as mr

    lib = C.CDLL(args.lib)
    lib.i8ie_last_error.restype = C.c_char_p
    P = C.c_void_p
    mr.bind(lib)
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]
    lib.i8ie_memcpy_d2h.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_mha.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

    ctx = P()
    ck(lib.i8ie_ctx_create(0, C.byref(ctx)))

    def alloc(nbytes):
        d = P()
        ck(lib.i8ie_malloc(ctx, nbytes, C.byref(d)))
        return d

    def put(arr):
        d = alloc(arr.nbytes)
        ck(lib.i8ie_memcpy_h2d(ctx, d, arr.ctypes.data_as(P), arr.nbytes))
        return d

    def get(d, shape):
        host = np.empty(shape, np.uint8)
        ck(lib.i8ie_memcpy_d2h(ctx, host.ctypes.data_as(P), d, host.nbytes))
        return host

    def timed(call):
        for _ in range(args.warmup):
            call()
        ck(lib.i8ie_sync(ctx))
        per_round, names = [], {}
        for _ in range(args.rounds):
            ck(lib.i8ie_profile_start(ctx, 0))
            for _ in range(args.iters):
                call()
            ents, cnt = (Entry * 64)(), C.c_int(0)
            ck(lib.i8ie_profile_stop(ctx, ents, 64, C.byref(cnt)))
            per_round.append(sum(ents[i].total_ms for i in range(cnt.value)) / args.iters)
            names = {ents[i].name.decode().split("|")[0]: int(ents[i].launches) // args.iters for i in range(cnt.value)}
        return {"ms": statistics.median(per_round), "ms_per_round": per_round, "kernels_per_call": names}

    results = []
    for name, t, c, heads in SHAPES:
        d = c // heads
        rng = np.random.default_rng(sum(map(ord, name)))
        s_s = f32(0.03)   # ~40 score steps of standard deviation: spread scores, many table entries in use
        s_qk = f32(np.sqrt(float(s_s) * 40.0 / (5476.0 * np.sqrt(d))))
        qp = dict(s_q=s_qk, zp_q=120, s_k=s_qk, zp_k=131, s_v=f32(0.04), zp_v=125, s_s=s_s, zp_s=140, s_o=f32(0.01), zp_o=128)
        for m in BATCHES:
            q, k, v = (rng.integers(0, 256, (m, t, c), dtype=np.uint8) for _ in range(3))
            dq, dk, dv = put(q), put(k), put(v)
            dsc, dpr, dfused, dcomp = alloc(m * t * t), alloc(m * t * t), alloc(m * t * c), alloc(m * t * c)
            g = mr.AttnArgs(b=m, heads=heads, d=d, tq=t, tk=t, q=mr.mat(dq.value, t, c), k=mr.mat(dk.value, t, c), v=mr.mat(dv.value, t, c),
                            out=mr.mat(dfused.value, t, c), **qp)
            per_head = []
            for h in range(heads):
                off = h * d
                s1 = ar.BmmArgs(b=m, m=t, n=t, k=d, a=ar.BmmMat(dq.value + off, t * c, c, 1, 0), bm=ar.BmmMat(dk.value + off, t * c, 1, c, 0),
                                out=ar.BmmMat(dsc.value, t * t, t, 1, 0), s_a=qp["s_q"], s_b=qp["s_k"], s_out=s_s, zp_a=qp["zp_q"],
                                zp_b=qp["zp_k"], zp_out=qp["zp_s"])
                s2 = ar.BmmArgs(b=m, m=t, n=d, k=t, a=ar.BmmMat(dpr.value, t * t, t, 1, 0), bm=ar.BmmMat(dv.value + off, t * c, c, 1, 0),
                                out=ar.BmmMat(dcomp.value + off, t * c, c, 1, 0), s_a=f32(1.0 / 256), s_b=qp["s_v"], s_out=qp["s_o"],
                                zp_a=0, zp_b=qp["zp_v"], zp_out=qp["zp_o"])
                per_head.append((s1, s2))

            def fused():
                ck(lib.i8ie_attention_u8(ctx, C.byref(g)))

            def composition():
                for s1, s2 in per_head:
                    ck(lib.i8ie_bmm_u8(ctx, C.byref(s1)))
                    ck(lib.i8ie_softmax_u8(ctx, dsc, dpr, m * t, t, s_s))
                    ck(lib.i8ie_bmm_u8(ctx, C.byref(s2)))

            fused()
            composition()
            got, comp = get(dfused, (m, t, c)), get(dcomp, (m, t, c))
            n = CHECKED_IMAGES
            want = mr.attention_u8(q[:n], k[:n], v[:n], heads, **qp)
            assert np.array_equal(got[:n], want[3]), "%s @ %d: the fused bytes differ from tests/mha_ref.py" % (name, m)
            assert np.array_equal(got, comp), "%s @ %d: the fused bytes differ from the composition's" % (name, m)
            rf, rc = timed(fused), timed(composition)
            ratio = rf["ms"] / rc["ms"]
            row = {"shape": name, "images": m, "t": t, "c": c, "heads": heads, "d": d, "identical_to_mha_ref_first_images": n,
                   "identical_to_composition": True, "scores_saturated_share": float(((want[0] == 0) | (want[0] == 255)).mean()),
                   "fused": rf, "composition": rc, "fused_over_composition": ratio, "spread": "+-3 %",
                   "aim_fused_le_composition": "met" if ratio <= 1.0 else "MISSED",
                   "fused_TOPS": 4.0 * m * heads * t * t * d / rf["ms"] / 1e9}
            for dev in (dq, dk, dv, dsc, dpr, dfused, dcomp):
                ck(lib.i8ie_free(ctx, dev))
            results.append(row)
            print(json.dumps(row), flush=True)
    lib.i8ie_ctx_destroy(ctx)
    return results


def network(args):
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx
    import i8ie
    from int8inferenceengine_amd import workloads as wl

    net = wl.calibrated("botnet_cifar", calib_batch=wl.synthetic_input("botnet_cifar", 16, seed=99))
    rows = []
    for m in BATCHES:
        x = i8ie.tensor(wl.synthetic_input("botnet_cifar", m)).prefetch()
        for _ in range(args.warmup):
            net(x).numpy()
        walls = []
        for _ in range(args.rounds):
            cx.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.net_steps):
                y = net(x)
            y.numpy()
            walls.append((time.perf_counter() - t0) / args.net_steps * 1e3)
        cx.profile_start()
        for _ in range(args.net_steps):
            net(x).numpy()
        prof = cx.profile_stop()
        total = sum(v[1] for v in prof.values())
        att = sum(v[1] for k, v in prof.items() if k.startswith("attn_"))
        by = {}
        for k, v in prof.items():
            by[k.split("|")[0]] = by.get(k.split("|")[0], 0.0) + v[1] / args.net_steps
        wall = statistics.median(walls)
        rows.append({"network": "botnet cifar (examples/botnet_cifar10.py)", "images": m, "step_ms_wall": wall, "step_ms_wall_per_round": walls,
                     "images_per_s_wall": m / (wall * 1e-3), "kernel_ms_per_step": total / args.net_steps,
                     "attention_ms_per_step": att / args.net_steps, "attention_share_of_kernel_time": att / total,
                     "attention_launches_per_step": sum(v[0] for k, v in prof.items() if k.startswith("attn_")) / args.net_steps,
                     "kernel_ms_per_step_by_name": by})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--net-steps", type=int, default=20)
    ap.add_argument("--lib", default=os.path.join(ROOT, "int8inferenceengine_amd", "libi8ie_hip.so"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"tool": "bench_mha", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "per-launch HIP events (i8ie_profile_*), summed per call; median over rounds of the per-round mean; spread +-3 %",
           "aim": "one fused i8ie_attention_u8 launch <= the 3 * H launches of i8ie_bmm_u8, i8ie_softmax_u8, i8ie_bmm_u8 per head",
           "results": kernels(args)}
    if args.net_steps > 0:
        out["network"] = network(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
