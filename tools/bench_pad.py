"""pad / crop against the cheapest pass over the same result: i8ie_relu_u8 on the result's byte count.

    python tools/bench_pad.py [--iters 10] [--rounds 3] [--warmup 3] [--net-steps 10] [--out profiles/r25_bench_pad.json]

Per case and batch size: i8ie_pad2d_u8_nhwc once into a flat plain result and once into a bordered (1) re-biased one, as a 3x3
pad-1 conv asks for it, with the relu folded in; and i8ie_relu_u8 over as many bytes as the result has, on the same build in the
same process.  A pad reads at most and writes exactly the result's byte count, as relu_u8 does, so the aim is the ratio <= 1.03
(3 % is the run-to-run spread); every row records the ratio and met / MISSED.  Timing is the library's own per-launch HIP-event
bracket (i8ie_profile_start / _stop): `warmup` calls unprofiled, then `rounds` rounds of `iters` profiled calls; a round's
figure is its mean per call and the reported one the median over rounds.  The flat results' first images are checked against
the index definition before the timing.  Then, through the Python surface: pad(reflect 1) -> conv3x3(padding=0) against the same
conv with padding=1 (other bytes, so only the times compare: the cost of the extra launch), and the INT8 step of
examples/cyclegan_generator_cifar10.py with the share of its kernel time in the pad kernels."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONSTANT, REFLECT, REPLICATE, CIRCULAR = 0, 1, 2, 3
AIM = 1.03

# (name, mode, c, h, w, (left, right, top, bottom)): the generator's residual blocks at two widths, its 7x7 stems, the
# asymmetric SAME padding of a stride-2 conv, and the original U-Net's centre crop
CASES = [("reflect1_128x8^2", REFLECT, 128, 8, 8, (1, 1, 1, 1)), ("reflect1_64x16^2", REFLECT, 64, 16, 16, (1, 1, 1, 1)),
         ("reflect3_32x32^2", REFLECT, 32, 32, 32, (3, 3, 3, 3)), ("constant0101_64x56^2", CONSTANT, 64, 56, 56, (0, 1, 0, 1)),
         ("crop_64x56^2_to_52^2", CONSTANT, 64, 56, 56, (-2, -2, -2, -2))]
CHAIN_CASES = [(128, 8), (64, 16)]
BATCHES = [1000, 125]
NEW_KERNELS = ("pad_u8_nhwc", "pad_u8_direct", "pad_f32")


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("total_ops", C.c_double),
                ("total_bytes", C.c_double)]


def definition(x, mode, amounts, fill):
    """the index rule of include/i8ie_hip.h on an NHWC tensor (numpy)"""
    def axis(L, before, after):
        src = []
        for o in range(L + before + after):
            i = o - before
            if 0 <= i < L:
                src.append(i)
            elif mode == CONSTANT:
                src.append(-1)
            elif mode == REFLECT:
                src.append(-i if i < 0 else 2 * (L - 1) - i)
            elif mode == REPLICATE:
                src.append(0 if i < 0 else L - 1)
            else:
                src.append(i + L if i < 0 else i - L)
        return np.asarray(src)

    l, r, t, b = amounts
    sy, sx = axis(x.shape[1], t, b), axis(x.shape[2], l, r)
    out = np.ascontiguousarray(x[:, np.maximum(sy, 0)[:, None], np.maximum(sx, 0)[None, :], :])
    out[:, (sy < 0)[:, None] | (sx < 0)[None, :], :] = fill
    return out


def kernels(args):
    lib = C.CDLL(args.lib)
    lib.i8ie_last_error.restype = C.c_char_p
    P, I, B = C.c_void_p, C.c_int, C.c_uint8
    lib.i8ie_pad2d_u8_nhwc.argtypes = [P, P, I, I, P, I, I] + [I] * 9 + [B, I, B]
    lib.i8ie_pad_output_shape.argtypes = [I] * 9 + [C.POINTER(I)]
    lib.i8ie_relu_u8.argtypes = [P, P, P, C.c_int64, B]
    lib.i8ie_fill_border_u8.argtypes = [P, P, I, I, I, I, I, B]
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]
    lib.i8ie_memcpy_d2h.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_pad.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

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

    zp, fill = 117, 117
    results = []
    for name, mode, c, h, w, amounts in CASES:
        rng = np.random.default_rng(sum(map(ord, name)))
        for m in BATCHES:
            dims = (I * 4)()
            ck(lib.i8ie_pad_output_shape(mode, *amounts, m, c, h, w, dims))
            _, _, oh, ow = tuple(dims)
            x = rng.integers(0, 256, (m, h, w, c), dtype=np.uint8)
            out_bytes = m * c * oh * ow
            dx = alloc(x.nbytes)
            ck(lib.i8ie_memcpy_h2d(ctx, dx, x.ctypes.data_as(P), x.nbytes))
            d_flat = alloc(out_bytes)
            d_bord = alloc(m * (oh + 2) * (ow + 2) * c)
            ck(lib.i8ie_fill_border_u8(ctx, d_bord, m, c, oh, ow, 1, zp ^ 0x80))
            row = {"case": name, "images": m, "c": c, "h": h, "w": w, "mode": mode, "amounts": list(amounts), "result": [c, oh, ow],
                   "result_bytes": out_bytes}
            ms, rounds, names = timed(lambda: ck(lib.i8ie_relu_u8(ctx, d_flat, d_flat, out_bytes, zp)))
            row["relu_u8_over_result_bytes"] = {"ms": ms, "ms_per_round": rounds, "kernels_per_call": names, "GBps": 2.0 * out_bytes / ms / 1e6}
            ck(lib.i8ie_pad2d_u8_nhwc(ctx, dx, 0, 0, d_flat, 0, 0, m, c, h, w, mode, *amounts, fill, 0, zp))
            k = min(m, 8)
            host = np.empty((k, oh, ow, c), np.uint8)
            ck(lib.i8ie_memcpy_d2h(ctx, host.ctypes.data_as(P), d_flat, host.nbytes))
            assert np.array_equal(host, definition(x[:k], mode, amounts, fill)), "%s @ %d: bytes differ from the definition" % (name, m)
            row["identical_to_definition"] = True
            for tag, dst, ob, s8 in (("flat", d_flat, 0, 0), ("bordered_rebiased", d_bord, 1, 1)):
                ms, rounds, names = timed(lambda: ck(lib.i8ie_pad2d_u8_nhwc(ctx, dx, 0, 0, dst, ob, s8, m, c, h, w, mode, *amounts, fill, 1, zp)))
                ratio = ms / row["relu_u8_over_result_bytes"]["ms"]
                row[tag] = {"ms": ms, "ms_per_round": rounds, "kernels_per_call": names, "GBps": 2.0 * out_bytes / ms / 1e6,
                            "over_relu_u8": ratio, "aim_at_most_1.03": "met" if ratio <= AIM else "MISSED"}
            for d in (dx, d_flat, d_bord):
                ck(lib.i8ie_free(ctx, d))
            results.append(row)
            print(json.dumps(row), flush=True)
    lib.i8ie_ctx_destroy(ctx)
    return results


def _profiled(cx, forward, steps):
    """(kernel ms per step, {kernel: ms per step}, {kernel: launches per step}) of `steps` calls of forward()"""
    cx.profile_start()
    for _ in range(steps):
        forward().numpy()
    prof = cx.profile_stop()
    by, launches = {}, {}
    for k, v in prof.items():
        by[k.split("|")[0]] = by.get(k.split("|")[0], 0.0) + v[1] / steps
        launches[k.split("|")[0]] = launches.get(k.split("|")[0], 0) + v[0] / steps
    return sum(by.values()), by, launches


def surface(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx
    import i8ie
    import cyclegan_generator_cifar10 as ex

    chains = []
    for c, hw in CHAIN_CASES:
        rng = np.random.default_rng(c)
        layers = {}
        for tag, padding in (("pad_then_conv_padding0", 0), ("conv_padding1", 1)):
            L = i8ie.Conv2d(c, c, 3, stride=1, padding=padding)
            L.load_weight((np.random.default_rng(c + 1).uniform(-1, 1, (c, c, 3, 3)) * np.sqrt(6.0 / (9 * c))).astype(np.float32))
            L.load_bias(np.zeros(c, np.float32))
            L.set_output_qparams(0.05, 120)
            L.convert()
            layers[tag] = L
        first = i8ie.Conv2d(c, c, 1)   # a producer, so that the operand is an NHWC activation as inside a network
        first.load_weight((rng.uniform(-1, 1, (c, c, 1, 1)) * np.sqrt(6.0 / c)).astype(np.float32))
        first.load_bias(np.zeros(c, np.float32))
        first.set_output_qparams(0.04, 110)
        first.convert()
        for m in BATCHES:
            q = i8ie.quantize(i8ie.tensor(rng.uniform(-2, 2, (m, c, hw, hw)).astype(np.float32)), 0.025, 127)
            row = {"case": "reflect1_conv3x3_%dx%d^2" % (c, hw), "images": m}
            forwards = {"pad_then_conv_padding0": lambda: layers["pad_then_conv_padding0"](i8ie.pad(first(q), (1, 1, 1, 1), "reflect")),
                        "conv_padding1": lambda: layers["conv_padding1"](first(q))}
            for tag, forward in forwards.items():
                for _ in range(args.warmup):
                    forward().numpy()
                per_round = []
                for _ in range(args.rounds):
                    total, by, launches = _profiled(cx, forward, args.iters)
                    per_round.append(total)
                row[tag] = {"kernel_ms": statistics.median(per_round), "kernel_ms_per_round": per_round, "kernel_ms_by_name": by,
                            "launches_by_name": launches}
            row["extra_launch_ms"] = row["pad_then_conv_padding0"]["kernel_ms"] - row["conv_padding1"]["kernel_ms"]
            chains.append(row)
            print(json.dumps(row), flush=True)

    model = ex.make_model(i8ie)
    model.load(ex.synthetic_state_dict(model))
    model.prepare()
    model(i8ie.tensor(np.random.default_rng(99).uniform(-1, 1, (16, 3, 32, 32)).astype(np.float32)))
    model.convert()
    rows = []
    for m in BATCHES:
        x = i8ie.tensor(np.random.default_rng(1234).uniform(-1, 1, (m, 3, 32, 32)).astype(np.float32)).prefetch()
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
        total, by, launches = _profiled(cx, lambda: model(x), args.net_steps)
        new = sum(v for k, v in by.items() if k in NEW_KERNELS)
        wall = statistics.median(walls)
        rows.append({"network": "examples/cyclegan_generator_cifar10.py", "images": m, "step_ms_wall": wall, "step_ms_wall_per_round": walls,
                     "images_per_s_wall": m / (wall * 1e-3), "kernel_ms_per_step": total, "pad_ms_per_step": new,
                     "pad_share_of_kernel_time": new / total, "kernel_ms_per_step_by_name": by, "launches_per_step_by_name": launches})
        print(json.dumps(rows[-1]), flush=True)
    return chains, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--net-steps", type=int, default=10)
    ap.add_argument("--lib", default=os.path.join(ROOT, "int8inferenceengine_amd", "libi8ie_hip.so"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"tool": "bench_pad", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "per-launch HIP events (i8ie_profile_*), summed per call; median over rounds of the per-round mean",
           "aim": "pad ms / relu_u8 ms over the result's byte count <= 1.03", "results": kernels(args)}
    if args.net_steps > 0:
        out["pad_conv_chain"], out["network"] = surface(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
