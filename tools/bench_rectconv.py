"""Rectangular Conv2d (1 x k / k x 1 at stride 1) against the only workaround there was: the dense square Conv2d whose k x k kernel
holds the line kernel in its middle row / column and zeros elsewhere (k times the MACs), on the same input.

    python tools/bench_rectconv.py [--iters 20] [--rounds 5] [--warmup 5] [--net-steps 10] [--out profiles/r20_bench_rectconv.json]

Every (shape, batch) runs in a child process of its own under a time limit; the first failure stops the run.  Per child: the
same u8 NHWC input (no border) through the rect handle (lconv_mfma), through the square handle of the embedded kernel -- output
bytes asserted identical -- and through the rect handle under the force-fallback option, which is the grouped route (bytes
asserted identical again).  Timing is the library's own per-launch HIP-event bracket (i8ie_profile_start / _stop) summed over
the kernels of a forward: `warmup` forwards unprofiled, then `rounds` rounds of `iters` profiled forwards; a round's figure is
its mean per forward and the reported one the median over rounds.  The aim, recorded per row as met / MISSED: the rect layer
takes no longer than the workaround, within the +-3 % spread of the project's measurements (ratio <= 1.03).  Then the step of
examples/inception_cifar10.py through the Python surface, with the share its rectangular layers take of the kernel time."""
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

# (name, c, kc, kh, kw, h, w); padding (k - 1) / 2 along the line
SHAPES = [
    ("1x7_128_17x17", 128, 128, 1, 7, 17, 17),
    ("7x1_128_17x17", 128, 128, 7, 1, 17, 17),
    ("1x7_192_17x17", 192, 192, 1, 7, 17, 17),
    ("7x1_192_17x17", 192, 192, 7, 1, 17, 17),
    ("1x3_384_8x8", 384, 384, 1, 3, 8, 8),
    ("3x1_384_8x8", 384, 384, 3, 1, 8, 8),
    # the example's own layers
    ("example_1x7_64_16x16", 64, 64, 1, 7, 16, 16),
    ("example_7x1_96_16x16", 96, 96, 7, 1, 16, 16),
    ("example_1x7_96_48_16x16", 96, 48, 1, 7, 16, 16),
    ("example_1x3_96_64_8x8", 96, 64, 1, 3, 8, 8),
    ("example_3x1_96_64_8x8", 96, 64, 3, 1, 8, 8),
]
BATCHES = [1000, 125]
CHILD_LIMIT_S = 240
AIM = 1.03


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("total_ops", C.c_double),
                ("total_bytes", C.c_double)]


class Geom(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("kh", "kw", "stride_h", "stride_w", "pad_h", "pad_w", "dilation_h", "dilation_w")]


def one_shape(args, shape, m):
    name, c, kc, kh, kw, h, w = shape
    lib = C.CDLL(args.lib)
    lib.i8ie_last_error.restype = C.c_char_p
    P, I, F = C.c_void_p, C.c_int, C.c_float
    lib.i8ie_conv2d_create.argtypes = [P, P, P, I, I, I, I, I, I, F, P]
    lib.i8ie_conv2d_create_rect.argtypes = [P, P, P, I, I, I, P, F, P]
    lib.i8ie_layer_forward_fused.argtypes = [P, P, I, I, I, I, I, F, C.c_uint8, I, P, I, I, P]
    lib.i8ie_layer_set_output_qparams.argtypes = [P, F, C.c_uint8]
    lib.i8ie_ctx_set_option.argtypes = [P, I, I]
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]
    lib.i8ie_memcpy_d2h.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_rectconv.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

    ctx = P()
    ck(lib.i8ie_ctx_create(0, C.byref(ctx)))
    s_in, zp_in, s_w, zp_out = 0.03, 121, 2e-3, 37
    rng = np.random.default_rng(sum(map(ord, name)))
    k = max(kh, kw)
    qw = rng.integers(-127, 128, (kc, c, kh, kw), dtype=np.int8)
    qws = np.zeros((kc, c, k, k), np.int8)  # the workaround's kernel: the line in the middle row / column of a k x k square
    if kh == 1:
        qws[:, :, k // 2:k // 2 + 1, :] = qw
    else:
        qws[:, :, :, k // 2:k // 2 + 1] = qw
    qb = rng.integers(-127, 128, kc, dtype=np.int8)
    s_out = float(np.float32(s_in * s_w * np.sqrt(c * k) * 74.0 * 73.0 / 20.0))
    g = Geom(kh, kw, 1, 1, kh // 2, kw // 2, 1, 1)
    L = P()
    ck(lib.i8ie_conv2d_create_rect(ctx, qw.ctypes.data_as(P), qb.ctypes.data_as(P), kc, c, 1, C.byref(g), s_w, C.byref(L)))
    Ls = P()
    ck(lib.i8ie_conv2d_create(ctx, qws.ctypes.data_as(P), qb.ctypes.data_as(P), kc, c, k, k, 1, k // 2, s_w, C.byref(Ls)))
    for x_ in (L, Ls):
        ck(lib.i8ie_layer_set_output_qparams(x_, s_out, zp_out))
    x = rng.integers(0, 256, (m, h, w, c), dtype=np.uint8)
    dx = P()
    ck(lib.i8ie_malloc(ctx, x.nbytes, C.byref(dx)))
    ck(lib.i8ie_memcpy_h2d(ctx, dx, x.ctypes.data_as(P), x.nbytes))
    row = {"shape": name, "images": m, "c": c, "kc": kc, "kh": kh, "kw": kw, "h": h, "w": w,
           "macs": m * h * w * kc * c * k, "macs_square_embedded": m * h * w * kc * c * k * k}
    outs = {}
    nbytes = m * h * w * kc
    for tag, handle, forced in (("rect", L, 0), ("square_embedded", Ls, 0), ("grouped_route", L, 1)):
        do = P()
        ck(lib.i8ie_malloc(ctx, nbytes, C.byref(do)))
        ck(lib.i8ie_ctx_set_option(ctx, 1, forced))

        def fwd():
            ck(lib.i8ie_layer_forward_fused(handle, dx, 1, 0, m, h, w, s_in, zp_in, 1, do, 1, 0, None))

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
        ck(lib.i8ie_ctx_set_option(ctx, 1, 0))
        host = np.empty(nbytes, np.uint8)
        ck(lib.i8ie_memcpy_d2h(ctx, host.ctypes.data_as(P), do, nbytes))
        outs[tag] = host
        ck(lib.i8ie_free(ctx, do))
        row[tag] = {"ms": statistics.median(per_round), "ms_per_round": per_round, "kernels_per_forward": names}
    assert np.array_equal(outs["rect"], outs["square_embedded"]), "%s @ %d: output bytes differ from the workaround's" % (name, m)
    assert np.array_equal(outs["rect"], outs["grouped_route"]), "%s @ %d: output bytes differ between the routes" % (name, m)
    assert any(n.startswith("lconv_mfma") for n in row["rect"]["kernels_per_forward"]), row["rect"]["kernels_per_forward"]
    row["identical_bytes"] = True
    row["rect_over_square_embedded"] = row["rect"]["ms"] / row["square_embedded"]["ms"]
    row["grouped_over_square_embedded"] = row["grouped_route"]["ms"] / row["square_embedded"]["ms"]
    row["aim"] = "met" if row["rect_over_square_embedded"] <= AIM else "MISSED"
    lib.i8ie_layer_destroy(L)
    lib.i8ie_layer_destroy(Ls)
    lib.i8ie_free(ctx, dx)
    lib.i8ie_ctx_destroy(ctx)
    print(json.dumps(row), flush=True)


def network(args, m):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx
    import i8ie
    import inception_cifar10 as ex

    net = ex.make_model(i8ie)
    net.load(ex.synthetic_state_dict(net))
    rng = np.random.default_rng(1234)
    net.prepare()
    net(i8ie.tensor(rng.standard_normal((16, 3, 32, 32)).astype(np.float32)))
    net.convert()
    x = i8ie.tensor(rng.standard_normal((m, 3, 32, 32)).astype(np.float32)).prefetch()
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
    by = {}
    for k, v in prof.items():
        by[k.split("|")[0]] = by.get(k.split("|")[0], 0.0) + v[1] / args.net_steps
    rect = by.get("lconv_mfma", 0.0)
    print(json.dumps({"network": "examples/inception_cifar10.py", "images": m, "step_ms_wall": wall, "kernel_ms_per_step": total / args.net_steps,
                      "images_per_s_wall": m / (wall * 1e-3), "lconv_ms_per_step": rect, "lconv_share_of_kernel_time": rect * args.net_steps / total,
                      "kernel_ms_per_step_by_name": by}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--net-steps", type=int, default=10)
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
    out = {"tool": "bench_rectconv", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup, "aim_ratio": AIM,
           "timing": "per-launch HIP events (i8ie_profile_*), summed per forward; median over rounds of the per-round mean",
           "results": [r for r in rows if "shape" in r], "network": [r for r in rows if "network" in r], "failed": failed}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    if failed:
        sys.exit("bench_rectconv.py: stopped at " + failed)


if __name__ == "__main__":
    main()
