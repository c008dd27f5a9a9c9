"""The padded / ceil-mode pools against the unpadded kernels the library already had, on the same input buffer in the same run.

    python tools/bench_padpool.py [--iters 20] [--rounds 5] [--warmup 5] [--out profiles/r19_bench_padpool.json]

At 1000 and 125 images, NHWC, border-free:
  max   i8ie_maxpool2d_u8_nhwc_pad at 3/2 padding 1 on [N, 64, 112, 112] (the ResNet stem) and at 3/2 ceil_mode on
        [N, 64, 56, 56] and [N, 256, 13, 13], beside i8ie_maxpool2d_u8_nhwc with the same window and stride at padding 0 on the
        same input: the same loads per output with no edge handling.
  avg   i8ie_avgpool2d_u8_nhwc_pad at 3/1 padding 1 on [N, 192, 28, 28] and [N, 64, 56, 56], beside i8ie_avgpool2d_u8_nhwc
        3x3 stride 1 on the same input.
The two legs of a row have different output sizes, so the figure compared is time per output byte; the aim is the yardstick's
within the project's +-3 % spread (met / MISSED per row).  The padded kernel's bytes of the first two images are asserted
against the definition (tests/padpool_ref.py) before anything is timed.
Timing is the library's own per-launch HIP-event bracket (i8ie_profile_start / _stop): `warmup` launches unprofiled, then
`rounds` rounds of `iters` profiled launches; a round's figure is its mean per launch, the reported one the median over
rounds.

Every measured shape runs in a child process of its own under a time limit, and the first failure stops the run: nothing
more is started on a device after a fault or a hang.  Goes through the C-ABI by ctypes only."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (kind, name, c, h, w, k, s, p, ceil_mode)
ROWS = [("max", "c64_112x112_3s2p1", 64, 112, 112, 3, 2, 1, 0), ("max", "c64_56x56_3s2ceil", 64, 56, 56, 3, 2, 0, 1),
        ("max", "c256_13x13_3s2ceil", 256, 13, 13, 3, 2, 0, 1), ("avg", "c192_28x28_3s1p1", 192, 28, 28, 3, 1, 1, 0),
        ("avg", "c64_56x56_3s1p1", 64, 56, 56, 3, 1, 1, 0)]
BATCHES = [1000, 125]
SPREAD = 1.03
STEP_TIMEOUT_S = 120


class Entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("total_ops", C.c_double),
                ("total_bytes", C.c_double)]


def run_case(args, kind, name, c, h, w, k, s, p, ceil_mode, m):
    import padpool_ref as ppr

    lib = ppr.bind(C.CDLL(args.lib))
    lib.i8ie_last_error.restype = C.c_char_p
    P, I, B = C.c_void_p, C.c_int, C.c_uint8
    lib.i8ie_avgpool2d_u8_nhwc.argtypes = [P, P, I, I, P, I, I] + [I] * 8 + [B]
    lib.i8ie_maxpool2d_u8_nhwc.argtypes = [P, P, I, P, I] + [I] * 6
    lib.i8ie_malloc.argtypes = [P, C.c_size_t, P]
    lib.i8ie_free.argtypes = [P, P]
    lib.i8ie_memcpy_h2d.argtypes = [P, P, P, C.c_size_t]
    lib.i8ie_memcpy_d2h.argtypes = [P, P, P, C.c_size_t]

    def ck(rc):
        if rc != 0:
            sys.exit("bench_padpool.py: rc=%d: %s" % (rc, lib.i8ie_last_error().decode()))

    ctx = P()
    ck(lib.i8ie_ctx_create(0, C.byref(ctx)))

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ck(lib.i8ie_sync(ctx))
        per_round, names = [], set()
        for _ in range(args.rounds):
            ck(lib.i8ie_profile_start(ctx, 0))
            for _ in range(args.iters):
                fn()
            ents, cnt = (Entry * 64)(), C.c_int(0)
            ck(lib.i8ie_profile_stop(ctx, ents, 64, C.byref(cnt)))
            assert sum(int(ents[i].launches) for i in range(cnt.value)) == args.iters
            names |= {ents[i].name.decode().split("|")[0] for i in range(cnt.value)}
            per_round.append(sum(ents[i].total_ms for i in range(cnt.value)) / args.iters)
        return statistics.median(per_round), per_round, sorted(names)

    rng = np.random.default_rng(m + c + h)
    x = rng.integers(0, 256, (m, h, w, c), dtype=np.uint8)
    n_in = x.size
    oh, ow = ppr.out_size(h, k, s, p, ceil_mode), ppr.out_size(w, k, s, p, ceil_mode)
    yh, yw = (h - k) // s + 1, (w - k) // s + 1
    n_out, n_yard = m * oh * ow * c, m * yh * yw * c
    dx, do = P(), P()
    ck(lib.i8ie_malloc(ctx, n_in, C.byref(dx)))
    ck(lib.i8ie_malloc(ctx, n_out, C.byref(do)))  # (the yardstick's result is no larger)
    ck(lib.i8ie_memcpy_h2d(ctx, dx, x.ctypes.data_as(P), n_in))
    zp = 97

    def padded():
        if kind == "max":
            ck(lib.i8ie_maxpool2d_u8_nhwc_pad(ctx, dx, 0, 0, do, 0, 0, m, c, h, w, k, s, p, ceil_mode, 0, zp))
        else:
            ck(lib.i8ie_avgpool2d_u8_nhwc_pad(ctx, dx, 0, 0, do, 0, 0, m, c, h, w, k, s, p, ceil_mode, 1, 0, zp))

    def yardstick():
        if kind == "max":
            ck(lib.i8ie_maxpool2d_u8_nhwc(ctx, dx, 0, do, 0, m, c, h, w, k, s))
        else:
            ck(lib.i8ie_avgpool2d_u8_nhwc(ctx, dx, 0, 0, do, 0, 0, m, c, h, w, k, k, s, 0, 0))

    # the bytes of the first two images against the definition
    padded()
    head = np.empty((2, oh, ow, c), np.uint8)
    ck(lib.i8ie_memcpy_d2h(ctx, head.ctypes.data_as(P), do, head.size))
    x2 = np.ascontiguousarray(x[:2].transpose(0, 3, 1, 2))
    want = ppr.max_pool2d_u8(x2, k, s, p, bool(ceil_mode)) if kind == "max" else ppr.avg_pool2d_u8(x2, k, s, p, bool(ceil_mode), True, False, zp)
    assert np.array_equal(head.transpose(0, 3, 1, 2), want), "bench_padpool.py: %s: bytes differ from the definition" % name

    row = {"kind": kind, "shape": name, "images": m, "c": c, "h": h, "w": w, "k": k, "s": s, "p": p, "ceil_mode": ceil_mode,
           "input_bytes": n_in, "bytes_checked": int(head.size)}
    for tag, fn, nb in (("padded", padded, n_out), ("yardstick", yardstick, n_yard), ("padded_again", padded, n_out)):
        ms, per_round, names = timed(fn)
        row[tag] = {"ms": ms, "ms_per_round": per_round, "output_bytes": nb, "ns_per_output_byte": ms * 1e6 / nb,
                    "gb_per_s": (n_in + nb) / (ms * 1e-3) / 1e9, "kernels": names}
    best = min(row["padded"]["ns_per_output_byte"], row["padded_again"]["ns_per_output_byte"])
    row["padded_over_yardstick_time_per_output_byte"] = best / row["yardstick"]["ns_per_output_byte"]
    row["aim"] = "met" if row["padded_over_yardstick_time_per_output_byte"] <= SPREAD else "MISSED"
    for d in (dx, do):
        ck(lib.i8ie_free(ctx, d))
    lib.i8ie_ctx_destroy(ctx)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lib", default=os.path.join(ROOT, "int8inferenceengine_amd", "libi8ie_hip.so"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help="internal: kind,name,c,h,w,k,s,p,ceil_mode,images -- one row, in this process")
    args = ap.parse_args()

    if args.case:
        f = args.case.split(",")
        run_case(args, f[0], f[1], *(int(v) for v in f[2:]))
        return

    results = []
    for row in ROWS:
        for m in BATCHES:
            cmd = [sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--rounds", str(args.rounds), "--warmup",
                   str(args.warmup), "--lib", args.lib, "--case", ",".join(str(v) for v in row + (m,))]
            try:
                done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_TIMEOUT_S)
            except subprocess.TimeoutExpired:
                sys.exit("bench_padpool.py: %s at %d images ran past %d s; stopping" % (row[1], m, STEP_TIMEOUT_S))
            if done.returncode != 0:
                sys.exit("bench_padpool.py: %s at %d images ended with status %d; stopping" % (row[1], m, done.returncode))
            r = json.loads(done.stdout.strip().splitlines()[-1])
            results.append(r)
            print("%-4s %-20s %5d images: padded %.4f ns/B, yardstick %.4f ns/B, ratio %.3f  %s"
                  % (r["kind"], r["shape"], m, min(r["padded"]["ns_per_output_byte"], r["padded_again"]["ns_per_output_byte"]),
                     r["yardstick"]["ns_per_output_byte"], r["padded_over_yardstick_time_per_output_byte"], r["aim"]), flush=True)

    out = {"tool": "bench_padpool", "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "per-launch HIP events (i8ie_profile_*); median over rounds of the per-round mean per launch",
           "aim": "time per output byte within %.2f x the unpadded kernel's on the same input" % SPREAD, "results": results}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
