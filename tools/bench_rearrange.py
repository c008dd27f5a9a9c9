"""narrow / channel_shuffle / pixel_shuffle / pixel_unshuffle against the cheapest pass over the same result: i8ie_relu_u8 on the
result's byte count.

    python tools/bench_rearrange.py [--iters 10] [--rounds 3] [--warmup 3] [--net-steps 10] [--out profiles/r21_bench_rearrange.json]

Per case and batch size: i8ie_rearrange_u8_nhwc once into a flat plain result and once into a bordered (1) re-biased one, as a
3x3 pad-1 conv asks for it, with the relu folded in; and i8ie_relu_u8 over as many bytes as the result has, on the same build in
the same process.  Every op reads and writes exactly the result's byte count, as relu_u8 does, so the aim is the ratio <= 1.03
(3 % is the run-to-run spread); every row records the ratio and met / MISSED.  Timing is the library's own per-launch HIP-event
bracket (i8ie_profile_start / _stop): `warmup` calls unprofiled, then `rounds` rounds of `iters` profiled calls; a round's
figure is its mean per call and the reported one the median over rounds.  The flat results' first images are checked against
the index definition before the timing.  Then examples/shufflenetv2_cifar10.py's INT8 step through the Python surface with the
share of its kernel time in the new kernels."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARROW, CHANNEL_SHUFFLE, PIXEL_SHUFFLE, PIXEL_UNSHUFFLE = 0, 1, 2, 3
AIM = 1.03

# (name, kind, c, h, w, p0, p1): the halves of ShuffleNetV2's three stage widths and of a 16-divisible one, the shuffles of the
# same maps, a sub-pixel head and two space-to-depth stems
CASES = []
for _c, _hw in ((116, 16), (232, 8), (464, 4), (128, 16)):
    CASES.append(("narrow_lo_%dx%d^2" % (_c, _hw), NARROW, _c, _hw, _hw, 0, _c // 2))
    CASES.append(("narrow_hi_%dx%d^2" % (_c, _hw), NARROW, _c, _hw, _hw, _c // 2, _c // 2))
for _c, _hw in ((116, 16), (232, 8), (464, 4), (128, 16)):
    CASES.append(("channel_shuffle2_%dx%d^2" % (_c, _hw), CHANNEL_SHUFFLE, _c, _hw, _hw, 2, 0))
CASES.append(("channel_shuffle4_128x16^2", CHANNEL_SHUFFLE, 128, 16, 16, 4, 0))
CASES.append(("pixel_shuffle2_256x16^2", PIXEL_SHUFFLE, 256, 16, 16, 2, 0))
CASES.append(("pixel_unshuffle2_64x32^2", PIXEL_UNSHUFFLE, 64, 32, 32, 2, 0))
CASES.append(("pixel_unshuffle2_3x32^2", PIXEL_UNSHUFFLE, 3, 32, 32, 2, 0))
BATCHES = [1000, 125]
NEW_KERNELS = ("narrow_u8_nhwc", "chanperm_u8_nhwc", "rearrange_u8_direct", "rearrange_u8_nchw")


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("total_ops", C.c_double),
                ("total_bytes", C.c_double)]


def definition(x, kind, p0, p1):
    """the index definition of include/i8ie_hip.h on an NHWC tensor (numpy)"""
    m, h, w, c = x.shape
    if kind == NARROW:
        return x[..., p0:p0 + p1]
    if kind == CHANNEL_SHUFFLE:
        co = np.arange(c)
        return x[..., (co % p0) * (c // p0) + co // p0]
    r = p0
    if kind == PIXEL_SHUFFLE:
        oc = c // (r * r)
        return x.reshape(m, h, w, oc, r, r).transpose(0, 1, 4, 2, 5, 3).reshape(m, h * r, w * r, oc)
    return x.reshape(m, h // r, r, w // r, r, c).transpose(0, 1, 3, 5, 2, 4).reshape(m, h // r, w // r, c * r * r)


def kernels(args):
    lib = C.CDLL(args.lib)
    lib.i8ie_last_error.restype = C.c_char_p
    P, I = C.c_void_p, C.c_int
    lib.i8ie_rearrange_u8_nhwc.argtypes = [P, P, I, I, P, I, I] + [I] * 8 + [C.c_uint8]
    lib.i8ie_rearrange_output_shape.argtypes = [I] * 7 + [C.POINTER(I)]
    lib.i8ie_relu_u8.argtypes = [P, P, P, C.c_int64, C.c_uint8]
    lib.i8ie_fill_border_u8.argtypes = [P, P, I, I, I, I, I, C.c_uint8]
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]
    lib.i8ie_memcpy_d2h.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_rearrange.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

    ctx = P()
    ck(lib.i8ie_ctx_create(0, C.byref(ctx)))

    def alloc(nbytes):
        d = P()
        ck(lib.i8ie_malloc(ctx, nbytes, C.byref(d)))
        return d

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
        return statistics.median(per_round), per_round, names

    zp = 117
    results = []
    for name, kind, c, h, w, p0, p1 in CASES:
        rng = np.random.default_rng(sum(map(ord, name)))
        for m in BATCHES:
            dims = (I * 4)()
            ck(lib.i8ie_rearrange_output_shape(kind, p0, p1, m, c, h, w, dims))
            _, oc, oh, ow = tuple(dims)
            x = rng.integers(0, 256, (m, h, w, c), dtype=np.uint8)
            out_bytes = m * oc * oh * ow
            dx = alloc(x.nbytes)
            ck(lib.i8ie_memcpy_h2d(ctx, dx, x.ctypes.data_as(P), x.nbytes))
            d_flat = alloc(out_bytes)
            d_bord = alloc(m * (oh + 2) * (ow + 2) * oc)
            ck(lib.i8ie_fill_border_u8(ctx, d_bord, m, oc, oh, ow, 1, zp ^ 0x80))
            row = {"case": name, "images": m, "c": c, "h": h, "w": w, "p0": p0, "p1": p1, "result": [oc, oh, ow], "result_bytes": out_bytes}
            ms, rounds, names = timed(lambda: ck(lib.i8ie_relu_u8(ctx, d_flat, d_flat, out_bytes, zp)))
            row["relu_u8_over_result_bytes"] = {"ms": ms, "ms_per_round": rounds, "kernels_per_call": names, "GBps": 2.0 * out_bytes / ms / 1e6}
            ck(lib.i8ie_rearrange_u8_nhwc(ctx, dx, 0, 0, d_flat, 0, 0, m, c, h, w, kind, p0, p1, 0, zp))
            k = min(m, 8)
            host = np.empty((k, oh, ow, oc), np.uint8)
            ck(lib.i8ie_memcpy_d2h(ctx, host.ctypes.data_as(P), d_flat, host.nbytes))
            assert np.array_equal(host, definition(x[:k], kind, p0, p1)), "%s @ %d: bytes differ from the definition" % (name, m)
            row["identical_to_definition"] = True
            for tag, dst, ob, s8 in (("flat", d_flat, 0, 0), ("bordered_rebiased", d_bord, 1, 1)):
                ms, rounds, names = timed(lambda: ck(lib.i8ie_rearrange_u8_nhwc(ctx, dx, 0, 0, dst, ob, s8, m, c, h, w, kind, p0, p1, 1, zp)))
                ratio = ms / row["relu_u8_over_result_bytes"]["ms"]
                row[tag] = {"ms": ms, "ms_per_round": rounds, "kernels_per_call": names, "GBps": 2.0 * out_bytes / ms / 1e6,
                            "over_relu_u8": ratio, "aim_at_most_1.03": "met" if ratio <= AIM else "MISSED"}
            for d in (dx, d_flat, d_bord):
                ck(lib.i8ie_free(ctx, d))
            results.append(row)
            print(json.dumps(row), flush=True)
    lib.i8ie_ctx_destroy(ctx)
    return results


def network(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx
    import i8ie
    import shufflenetv2_cifar10 as ex

    model = ex.make_model(i8ie)
    model.load(ex.synthetic_state_dict(model))
    model.prepare()
    model(i8ie.tensor(np.random.default_rng(99).standard_normal((16, 3, 32, 32)).astype(np.float32)))
    model.convert()
    rows = []
    for m in BATCHES:
        x = i8ie.tensor(np.random.default_rng(1234).standard_normal((m, 3, 32, 32)).astype(np.float32)).prefetch()
        for _ in range(args.warmup):
            model(x).numpy()
        walls = []
        for _ in range(args.rounds):
            cx.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.net_steps):
                y = model(x)
            y.numpy()
            walls.append((time.perf_counter() - t0) / args.net_steps * 1e3)
        cx.profile_start()
        for _ in range(args.net_steps):
            model(x).numpy()
        prof = cx.profile_stop()
        total = sum(v[1] for v in prof.values())
        by, launches = {}, {}
        for k, v in prof.items():
            by[k.split("|")[0]] = by.get(k.split("|")[0], 0.0) + v[1] / args.net_steps
            launches[k.split("|")[0]] = launches.get(k.split("|")[0], 0) + v[0] / args.net_steps
        new = sum(v for k, v in by.items() if k in NEW_KERNELS)
        wall = statistics.median(walls)
        rows.append({"network": "examples/shufflenetv2_cifar10.py", "images": m, "step_ms_wall": wall, "step_ms_wall_per_round": walls,
                     "images_per_s_wall": m / (wall * 1e-3), "kernel_ms_per_step": total / args.net_steps,
                     "rearrange_ms_per_step": new, "rearrange_share_of_kernel_time": new / (total / args.net_steps),
                     "kernel_ms_per_step_by_name": by, "launches_per_step_by_name": launches})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--net-steps", type=int, default=10)
    ap.add_argument("--lib", default=os.path.join(ROOT, "int8inferenceengine_amd", "libi8ie_hip.so"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"tool": "bench_rearrange", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "per-launch HIP events (i8ie_profile_*), summed per call; median over rounds of the per-round mean",
           "aim": "rearrange ms / relu_u8 ms over the result's byte count <= 1.03", "results": kernels(args)}
    if args.net_steps > 0:
        out["network"] = network(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
