"""The shifted-window attention against the windowed attention on the same buffers.

    python tools/bench_swin.py [--iters 20] [--rounds 5] [--warmup 5] [--net-steps 10] [--out profiles/r28_bench_swin.json]

Per shape of tools/bench_window_attention.py (an h x w map of c = H * d channels, wh x ww windows) and at 1000 and 125 images:
ONE i8ie_attention_swin_u8 launch on the packed channels-last map [n, h, w, 3c] in each of three forms -- shift only
(shift = window // 2), bias only, shift + bias -- against the yardstick, ONE i8ie_attention_window_u8 launch (no shift, no
bias) on the same buffers in the same process.  The aim is form / yardstick <= 1.03 (the run-to-run spread of these figures is
about +-3 %); a miss is reported as MISSED.  Timing is bench_window_attention.py's: the library's own per-launch HIP-event
bracket, `warmup` calls unprofiled, then `rounds` rounds of `iters` profiled calls; a round's figure is its mean per call and
the reported one the median over rounds.  Before the timing the shift + bias result of the first image is asserted against
tests/swin_ref.py (the numpy definition), and the swin entry with shift 0 and no bias against the yardstick's bytes.  Then the
step of examples/swin_cifar10.py through the Python surface with the share its shifted-window launches take."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "examples"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
from bench_window_attention import AIM, BATCHES, SHAPES, Entry  # noqa: E402

f32 = np.float32
FORMS = ("shift_only", "bias_only", "shift_and_bias")


def kernels(args):
    import mha_ref as mr
    import swin_ref as sr
    import window_ref as wr

    lib = C.CDLL(args.lib)
    lib.i8ie_last_error.restype = C.c_char_p
    P = C.c_void_p
    sr.bind(lib)
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]
    lib.i8ie_memcpy_d2h.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_swin.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

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
    for name, side, c, win, heads in SHAPES:
        d, T = c // heads, win * win
        rng = np.random.default_rng(sum(map(ord, name)))
        s_s = f32(0.03)
        s_qk = f32(np.sqrt(float(s_s) * 40.0 / (5476.0 * np.sqrt(d))))
        qp = dict(s_q=s_qk, zp_q=120, s_k=s_qk, zp_k=120, s_v=s_qk, zp_v=120, s_s=s_s, zp_s=140, s_o=f32(0.01), zp_o=128)
        bias = sr.expand_bias(rng.normal(0, 0.5, ((2 * win - 1) ** 2, heads)).astype(f32), win)
        dbias = put(sr.padded_bias(bias))
        for m in BATCHES:
            x = rng.integers(0, 256, (m, side, side, 3 * c), dtype=np.uint8)     # the packed map, channels last
            dx, dout, dyard = put(x), alloc(m * side * side * c), alloc(m * side * side * c)
            mk = lambda out: mr.AttnArgs(b=m, heads=heads, d=d, tq=T, tk=T, out=wr.map_mat(out.value, side, side, c), out_h=side, out_w=side,  # noqa: E731
                                         **{o: wr.map_mat(dx.value, side, side, 3 * c, offset=i * c) for i, o in enumerate("qkv")}, **qp)
            g, y = mk(dout), mk(dyard)
            w = wr.AttnWindow(map_h=side, map_w=side, win_h=win, win_w=win)
            half = win // 2
            forms = {"shift_only": sr.AttnSwin(half, half, None), "bias_only": sr.AttnSwin(0, 0, dbias.value),
                     "shift_and_bias": sr.AttnSwin(half, half, dbias.value), "neither": sr.AttnSwin(0, 0, None)}

            def swin(form):
                return lambda: ck(lib.i8ie_attention_swin_u8(ctx, C.byref(g), C.byref(w), C.byref(forms[form])))

            def yardstick():
                ck(lib.i8ie_attention_window_u8(ctx, C.byref(y), C.byref(w)))

            yardstick()
            swin("neither")()
            assert np.array_equal(get(dout, (m, side, side, c)), get(dyard, (m, side, side, c))), "%s @ %d: shift 0, no bias differs from the yardstick" % (name, m)
            swin("shift_and_bias")()
            want = sr.attention_u8(np.ascontiguousarray(x[:1].transpose(0, 3, 1, 2)), None, None, heads, win, half, bias, **qp)
            assert np.array_equal(get(dout, (m, side, side, c))[:1].transpose(0, 3, 1, 2), want[3]), "%s @ %d: differs from tests/swin_ref.py" % (name, m)
            ry = timed(yardstick)
            row = {"shape": name, "images": m, "map": [side, side], "c": c, "window": [win, win], "shift": [half, half], "heads": heads, "d": d,
                   "identical_to_swin_ref_first_image": True, "shift0_no_bias_identical_to_yardstick": True, "yardstick": ry, "spread": "+-3 %"}
            for form in FORMS:
                r = timed(swin(form))
                ratio = r["ms"] / ry["ms"]
                row[form] = r
                row[form + "_over_yardstick"] = ratio
                row["aim_%s_over_yardstick_le_1.03" % form] = "met" if ratio <= AIM else "MISSED"
            for dev in (dx, dout, dyard):
                ck(lib.i8ie_free(ctx, dev))
            results.append(row)
            print(json.dumps(row), flush=True)
        ck(lib.i8ie_free(ctx, dbias))
    lib.i8ie_ctx_destroy(ctx)
    return results


def network(args):
    import int8inferenceengine_amd  # noqa: F401
    import _CXX_i8ie as cx
    import i8ie
    import swin_cifar10 as sw

    net = sw.make_model(i8ie)
    net.load(sw.synthetic_state_dict())
    net.prepare()
    net(i8ie.tensor(np.random.default_rng(99).uniform(-1, 1, (16, 3, 32, 32)).astype(f32)))
    net.convert()
    rows = []
    for m in BATCHES:
        x = i8ie.tensor(np.random.default_rng(1234).uniform(-1, 1, (m, 3, 32, 32)).astype(f32)).prefetch()
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
        is_swin = lambda k: k.split("|")[0] in sw.SWIN_KERNELS  # noqa: E731
        att = sum(v[1] for k, v in prof.items() if is_swin(k))
        wall = statistics.median(walls)
        rows.append({"network": "swin cifar (examples/swin_cifar10.py)", "images": m, "step_ms_wall": wall, "step_ms_wall_per_round": walls,
                     "images_per_s_wall": m / (wall * 1e-3), "kernel_ms_per_step": total / args.net_steps,
                     "swin_attention_ms_per_step": att / args.net_steps, "swin_attention_share_of_kernel_time": att / total,
                     "swin_attention_launches_per_step": sum(v[0] for k, v in prof.items() if is_swin(k)) / args.net_steps})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--net-steps", type=int, default=10)
    ap.add_argument("--lib", default=os.path.join(ROOT, "int8inferenceengine_amd", "libi8ie_hip.so"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"tool": "bench_swin", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup, "batches": BATCHES,
           "timing": "per-launch HIP events (i8ie_profile_*), summed per call; median over rounds of the per-round mean; spread +-3 %",
           "yardstick": "i8ie_attention_window_u8 (no shift, no bias) on the same buffers in the same process",
           "aim": "form / yardstick <= 1.03, stamped met / MISSED on all three forms (shift only moves the same bytes; the bias forms read 4 T^2 more bytes per (window, head))",
           "results": kernels(args)}
    if args.net_steps > 0:
        out["network"] = network(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
