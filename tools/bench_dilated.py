"""Dilated Conv2d against (a) the only workaround there was, a dense Conv2d whose kernel is inflated with zeros, and (b) the same
layer at dilation 1 on the tuned route (equal MACs).

    python tools/bench_dilated.py [--iters 20] [--rounds 5] [--warmup 5] [--net-steps 20] [--out profiles/r14_bench_dilated.json]

Every (shape, batch) runs in a child process of its own under a time limit; the first failure stops the run.  Per child: the
same u8 NHWC input (no border) through the dilated handle, through the dense handle of the inflated weights -- output bytes
asserted identical -- and, for dense shapes, through the handle of the same weights at dilation 1 with padding (k - 1) / 2.
Timing is the library's own per-launch HIP-event bracket (i8ie_profile_start / _stop) summed over the kernels of a forward:
`warmup` forwards unprofiled, then `rounds` rounds of `iters` profiled forwards; a round's figure is its mean per forward and
the reported one the median over rounds.  Then deeplabv3_cifar's step through the Python surface, with the share its dilated
layers take of the kernel time."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, c, kc, groups, k, pad, dilation, h, w)
SHAPES = [
    ("deeplab_s4b1c1_256_512_d2_8x8", 256, 512, 1, 3, 2, 2, 8, 8),
    ("deeplab_s4_512_512_d2_8x8", 512, 512, 1, 3, 2, 2, 8, 8),
    ("deeplab_aspp_512_128_d2_8x8", 512, 128, 1, 3, 2, 2, 8, 8),
    ("deeplab_aspp_512_128_d4_8x8", 512, 128, 1, 3, 4, 4, 8, 8),
    ("deeplab_aspp_512_128_d6_8x8", 512, 128, 1, 3, 6, 6, 8, 8),
    ("64_64_d2_56x56", 64, 64, 1, 3, 2, 2, 56, 56),
    ("depthwise_256_d2_16x16", 256, 256, 256, 3, 2, 2, 16, 16),
]
BATCHES = [1000, 125]
CHILD_LIMIT_S = 240


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("total_ops", C.c_double),
                ("total_bytes", C.c_double)]


def inflate(w, d):
    out = np.zeros(w.shape[:-2] + (d * (w.shape[-2] - 1) + 1, d * (w.shape[-1] - 1) + 1), w.dtype)
    out[..., ::d, ::d] = w
    return out


def one_shape(args, shape, m):
    name, c, kc, g, k, p, d, h, w = shape
    lib = C.CDLL(args.lib)
    lib.i8ie_last_error.restype = C.c_char_p
    P, I, F = C.c_void_p, C.c_int, C.c_float
    lib.i8ie_conv2d_create_grouped.argtypes = [P, P, P, I, I, I, I, I, I, I, F, P]
    lib.i8ie_conv2d_create_dilated.argtypes = [P, P, P, I, I, I, I, I, I, I, I, F, P]
    lib.i8ie_layer_forward_fused.argtypes = [P, P, I, I, I, I, I, F, C.c_uint8, I, P, I, I, P]
    lib.i8ie_layer_set_output_qparams.argtypes = [P, F, C.c_uint8]
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]
    lib.i8ie_memcpy_d2h.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_dilated.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

    ctx = P()
    ck(lib.i8ie_ctx_create(0, C.byref(ctx)))
    s_in, zp_in, s_w, zp_out = 0.03, 121, 2e-3, 37
    rng = np.random.default_rng(sum(map(ord, name)))
    Cg = c // g
    qw = rng.integers(-127, 128, (kc, Cg, k, k), dtype=np.int8)
    qwi = np.ascontiguousarray(inflate(qw, d))
    qb = rng.integers(-127, 128, kc, dtype=np.int8)
    s_out = float(np.float32(s_in * s_w * np.sqrt(Cg * k * k) * 74.0 * 73.0 / 20.0))
    ke = d * (k - 1) + 1
    oh, ow = h + 2 * p - ke + 1, w + 2 * p - ke + 1
    layers = {}
    L = P()
    ck(lib.i8ie_conv2d_create_dilated(ctx, qw.ctypes.data_as(P), qb.ctypes.data_as(P), kc, c, k, k, 1, p, g, d, s_w, C.byref(L)))
    layers["dilated"] = (L, oh, ow)
    L = P()
    ck(lib.i8ie_conv2d_create_grouped(ctx, qwi.ctypes.data_as(P), qb.ctypes.data_as(P), kc, c, ke, ke, 1, p, g, s_w, C.byref(L)))
    layers["dense_inflated"] = (L, oh, ow)
    L = P()
    ck(lib.i8ie_conv2d_create_grouped(ctx, qw.ctypes.data_as(P), qb.ctypes.data_as(P), kc, c, k, k, 1, (k - 1) // 2, g, s_w, C.byref(L)))
    layers["dilation_1"] = (L, h, w)
    for L, _, _ in layers.values():
        ck(lib.i8ie_layer_set_output_qparams(L, s_out, zp_out))
    x = rng.integers(0, 256, (m, h, w, c), dtype=np.uint8)
    dx = P()
    ck(lib.i8ie_malloc(ctx, x.nbytes, C.byref(dx)))
    ck(lib.i8ie_memcpy_h2d(ctx, dx, x.ctypes.data_as(P), x.nbytes))
    row = {"shape": name, "images": m, "c": c, "kc": kc, "groups": g, "kernel": k, "pad": p, "dilation": d, "h": h, "w": w,
           "macs": m * oh * ow * kc * Cg * k * k, "macs_dense_inflated": m * oh * ow * kc * Cg * ke * ke}
    outs = {}
    for tag, (L, o_h, o_w) in layers.items():
        nbytes = m * o_h * o_w * kc
        do = P()
        ck(lib.i8ie_malloc(ctx, nbytes, C.byref(do)))

        def fwd():
            ck(lib.i8ie_layer_forward_fused(L, dx, 1, 0, m, h, w, s_in, zp_in, 1, do, 1, 0, None))

        for _ in range(args.warmup):
            fwd()
        ck(lib.i8ie_sync(ctx))
        per_round, names = [], {}
        for _ in range(args.rounds):
            ck(lib.i8ie_profile_start(ctx, 0))
            for _ in range(args.iters):
                fwd()
            ents, cnt = (Entry * 64)(), C.c_int(0)
            ck(lib.i8ie_profile_stop(ctx, ents, 64, C.byref(cnt)))
            per_round.append(sum(ents[i].total_ms for i in range(cnt.value)) / args.iters)
            names = {ents[i].name.decode(): int(ents[i].launches) // args.iters for i in range(cnt.value)}
        host = np.empty(nbytes, np.uint8)
        ck(lib.i8ie_memcpy_d2h(ctx, host.ctypes.data_as(P), do, nbytes))
        outs[tag] = host
        ck(lib.i8ie_free(ctx, do))
        row[tag] = {"ms": statistics.median(per_round), "ms_per_round": per_round, "kernels_per_forward": names}
    assert np.array_equal(outs["dilated"], outs["dense_inflated"]), "%s @ %d: output bytes differ" % (name, m)
    row["identical_bytes"] = True
    row["dilated_over_dense_inflated"] = row["dilated"]["ms"] / row["dense_inflated"]["ms"]
    row["dilated_over_dilation_1"] = row["dilated"]["ms"] / row["dilation_1"]["ms"]
    for L, _, _ in layers.values():
        lib.i8ie_layer_destroy(L)
    lib.i8ie_free(ctx, dx)
    lib.i8ie_ctx_destroy(ctx)
    print(json.dumps(row), flush=True)


def network(args, m):
    sys.path.insert(0, ROOT)
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx
    import i8ie
    from int8inferenceengine_amd import workloads as wl

    name = "deeplabv3_cifar"
    net = wl.calibrated(name, calib_batch=wl.synthetic_input(name, 16, seed=99))
    x = i8ie.tensor(wl.synthetic_input(name, m)).prefetch()
    for _ in range(args.warmup):
        net(x).numpy()
    cx.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.net_steps):
        y = net(x)
    y.numpy()
    wall = (time.perf_counter() - t0) / args.net_steps * 1e3
    cx.profile_start()
    for _ in range(args.net_steps):
        net(x).numpy()
    prof = cx.profile_stop()
    total = sum(v[1] for v in prof.values())
    dil = sum(v[1] for k, v in prof.items() if k.startswith(("dconv", "gconv")))  # (the network has no grouped layer: these are its dilated layers)
    by = {}
    for k, v in prof.items():
        by[k.split("|")[0]] = by.get(k.split("|")[0], 0.0) + v[1] / args.net_steps
    print(json.dumps({"network": name, "images": m, "step_ms_wall": wall, "kernel_ms_per_step": total / args.net_steps,
                      "images_per_s_wall": m / (wall * 1e-3), "dilated_ms_per_step": dil / args.net_steps,
                      "dilated_share_of_kernel_time": dil / total, "kernel_ms_per_step_by_name": by}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--net-steps", type=int, default=20)
    ap.add_argument("--lib", default=os.path.join(ROOT, "int8inferenceengine_amd", "libi8ie_hip.so"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help="internal: 'shape:<index>:<images>' or 'net:<images>'")
    args = ap.parse_args()
    if args.child:
        kind, *rest = args.child.split(":")
        if kind == "shape":
            one_shape(args, SHAPES[int(rest[0])], int(rest[1]))
        else:
            network(args, int(rest[0]))
        return
    jobs = ["shape:%d:%d" % (i, m) for i in range(len(SHAPES)) for m in BATCHES]
    if args.net_steps > 0:
        jobs += ["net:%d" % m for m in BATCHES]
    rows, failed = [], None
    for job in jobs:  # a fresh process per job, under its own limit; nothing more is started after a failure
        cmd = [sys.executable, os.path.abspath(__file__), "--child", job, "--iters", str(args.iters), "--rounds", str(args.rounds),
               "--warmup", str(args.warmup), "--net-steps", str(args.net_steps), "--lib", args.lib]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            failed = "%s: time limit" % job
            break
        if r.returncode != 0:
            failed = "%s: exit status %d" % (job, r.returncode)
            break
        rows.append(json.loads(r.stdout.decode().strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), flush=True)
    out = {"tool": "bench_dilated", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "per-launch HIP events (i8ie_profile_*), summed per forward; median over rounds of the per-round mean",
           "results": [r for r in rows if "shape" in r], "network": [r for r in rows if "network" in r], "failed": failed}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    if failed:
        sys.exit("bench_dilated.py: stopped at " + failed)


if __name__ == "__main__":
    main()
