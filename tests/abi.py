"""ctypes binding of libi8ie_hip.so used by the tests (and a model of the stub an
FFI user would write).  numpy in, numpy out; every call goes
through the C-ABI declared in include/i8ie_hip.h."""
import contextlib
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# ($I8IE_LIB: another build of the same C-ABI, e.g. an A/B build of tools/dbg/build_ab.sh)
LIB_PATH = os.environ.get("I8IE_LIB") or os.path.join(ROOT, "int8inferenceengine_amd", "libi8ie_hip.so")
HEADER = os.path.join(ROOT, "include", "i8ie_hip.h")

_lib = None


def declared_symbols():
    """Every function name declared in include/i8ie_hip.h."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(i8ie_[a-z0-9_]+)\s*\(", src)))


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libi8ie_hip.so not built: run python -m int8inferenceengine_amd.build")
        _lib = C.CDLL(LIB_PATH)
        _lib.i8ie_last_error.restype = C.c_char_p
        _lib.i8ie_ctx_stream.restype = C.c_void_p
    return _lib


class AbiError(RuntimeError):
    pass


def ck(rc):
    if rc != 0:
        raise AbiError("rc=%d: %s" % (rc, lib().i8ie_last_error().decode()))


class Dev:
    """A device buffer with shape/dtype bookkeeping."""

    def __init__(self, ctx, shape, dtype):
        self.ctx, self.shape, self.dtype = ctx, tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.ptr = C.c_void_p()
        ck(lib().i8ie_malloc(ctx.h, C.c_size_t(self.nbytes), C.byref(self.ptr)))

    def get(self):
        out = np.empty(self.shape, self.dtype)
        ck(lib().i8ie_memcpy_d2h(self.ctx.h, out.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(self.nbytes)))
        return out

    def free(self):
        if self.ptr:
            lib().i8ie_free(self.ctx.h, self.ptr)
            self.ptr = C.c_void_p()


class GuardedOut:
    """A float32 output region with GUARD floats before and after it in one device allocation.  The guards are
    pre-filled with GUARD_BITS and the region with FILL_BITS (a quiet NaN no arithmetic here produces), so a store
    outside the region and an element never stored both show.  `ptr` is the region's address; read() returns
    (region, guards untouched?)."""
    GUARD = 4096
    GUARD_BITS = 0xA5C3F00D
    FILL_BITS = 0x7FC0DEAD

    def __init__(self, ctx, shape):
        self.shape = tuple(int(d) for d in shape)
        self.size = int(np.prod(self.shape, dtype=np.int64))
        host = np.full(self.size + 2 * self.GUARD, self.GUARD_BITS, np.uint32)
        host[self.GUARD:self.GUARD + self.size] = self.FILL_BITS
        self.buf = ctx.put(host)
        self.ptr = C.c_void_p(self.buf.ptr.value + 4 * self.GUARD)

    def read(self):
        bits = self.buf.get()
        g = self.GUARD
        ok = bool((bits[:g] == self.GUARD_BITS).all() and (bits[g + self.size:] == self.GUARD_BITS).all())
        return bits[g:g + self.size].view(np.float32).reshape(self.shape).copy(), ok

    @classmethod
    def unwritten(cls, out):
        """number of elements of a read() result that still hold the fill pattern"""
        return int((np.ascontiguousarray(out, np.float32).view(np.uint32) == cls.FILL_BITS).sum())

    def free(self):
        self.buf.free()


class GuardedU8:
    """The byte counterpart of GuardedOut: a region of `shape` elements of `dtype` with GUARD bytes before and after it
    in one device allocation, the guards pre-filled with GUARD_BYTE and the region with `fill`.  GUARD is a multiple of
    256, so `ptr` is aligned like an allocation of its own.  get() returns the region, guards_ok() whether no byte of
    either guard changed."""
    GUARD = 4096
    GUARD_BYTE = 0x5A

    def __init__(self, ctx, shape, dtype=np.uint8, fill=0xC3):
        self.shape, self.dtype = tuple(int(d) for d in shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        host = np.full(self.nbytes + 2 * self.GUARD, self.GUARD_BYTE, np.uint8)
        host[self.GUARD:self.GUARD + self.nbytes] = fill
        self.buf = ctx.put(host)
        self.ptr = C.c_void_p(self.buf.ptr.value + self.GUARD)
        self._raw = None

    def get(self):
        self._raw = self.buf.get()
        return self._raw[self.GUARD:self.GUARD + self.nbytes].view(self.dtype).reshape(self.shape).copy()

    def guards_ok(self):
        raw = self._raw if self._raw is not None else self.buf.get()
        g = self.GUARD
        return bool((raw[:g] == self.GUARD_BYTE).all() and (raw[g + self.nbytes:] == self.GUARD_BYTE).all())

    def free(self):
        self.buf.free()


class ProfEntry(C.Structure):
    """i8ie_profile_entry of include/i8ie_hip.h"""
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double),
                ("total_ops", C.c_double), ("total_bytes", C.c_double)]


class Ctx:
    def __init__(self, device=0):
        self.h = C.c_void_p()
        ck(lib().i8ie_ctx_create(device, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().i8ie_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        d = Dev(self, arr.shape, arr.dtype)
        ck(lib().i8ie_memcpy_h2d(self.h, d.ptr, arr.ctypes.data_as(C.c_void_p), C.c_size_t(d.nbytes)))
        return d

    def empty(self, shape, dtype):
        return Dev(self, shape, dtype)

    def sync(self):
        ck(lib().i8ie_sync(self.h))

    # ---- ops ---------------------------------------------------------------
    def quantize(self, x, scale, zp):
        x = np.ascontiguousarray(x, np.float32)
        d, o = self.put(x), self.empty(x.shape, np.uint8)
        ck(lib().i8ie_quantize_f32_u8(self.h, d.ptr, o.ptr, C.c_int64(x.size), C.c_float(scale), C.c_uint8(zp)))
        r = o.get()
        d.free(); o.free()
        return r

    def dequantize(self, q, scale, zp):
        q = np.ascontiguousarray(q, np.uint8)
        d, o = self.put(q), self.empty(q.shape, np.float32)
        ck(lib().i8ie_dequantize_u8_f32(self.h, d.ptr, o.ptr, C.c_int64(q.size), C.c_float(scale), C.c_uint8(zp)))
        r = o.get()
        d.free(); o.free()
        return r

    def down_scale(self, acc, sa, sb, sc, zp):
        acc = np.ascontiguousarray(acc, np.int32)
        d, o = self.put(acc), self.empty(acc.shape, np.uint8)
        ck(lib().i8ie_down_scale(self.h, d.ptr, o.ptr, C.c_int64(acc.size), C.c_float(sa), C.c_float(sb),
                                 C.c_float(sc), C.c_uint8(zp)))
        r = o.get()
        d.free(); o.free()
        return r

    def relu(self, q, zp):
        q = np.ascontiguousarray(q, np.uint8)
        d, o = self.put(q), self.empty(q.shape, np.uint8)
        ck(lib().i8ie_relu_u8(self.h, d.ptr, o.ptr, C.c_int64(q.size), C.c_uint8(zp)))
        r = o.get()
        d.free(); o.free()
        return r

    def max_pool2d(self, q, k, s):
        q = np.ascontiguousarray(q, np.uint8)
        n, c, h, w = q.shape
        oh, ow = (h - k) // s + 1, (w - k) // s + 1
        d, o = self.put(q), self.empty((n, c, oh, ow), np.uint8)
        ck(lib().i8ie_maxpool2d_u8(self.h, d.ptr, o.ptr, n, c, h, w, k, s))
        r = o.get()
        d.free(); o.free()
        return r

    def conv_offsets(self, qw, qb, s_in, zp_in):
        qw = np.ascontiguousarray(qw, np.int8)
        kc = qw.shape[0]
        K = qw.size // kc
        dw, db, o = self.put(qw), self.put(np.ascontiguousarray(qb, np.int8)), self.empty((kc,), np.int32)
        ck(lib().i8ie_conv_offsets(self.h, dw.ptr, db.ptr, kc, K, C.c_float(s_in), C.c_uint8(zp_in), o.ptr))
        r = o.get()
        dw.free(); db.free(); o.free()
        return r

    def linear_offsets(self, qw, zp_in):
        qw = np.ascontiguousarray(qw, np.int8)
        n, k = qw.shape
        dw, o = self.put(qw), self.empty((n,), np.int32)
        ck(lib().i8ie_linear_offsets(self.h, dw.ptr, n, k, C.c_uint8(zp_in), o.ptr))
        r = o.get()
        dw.free(); o.free()
        return r

    def linear(self, q_in, qw, qb, s_in, zp_in, s_w, s_out, zp_out, want_acc=True):
        """Stateless i8ie_linear_u8s8.  Returns (out, acc or None, oc)."""
        q_in = np.ascontiguousarray(q_in, np.uint8)
        qw = np.ascontiguousarray(qw, np.int8)
        qb = np.ascontiguousarray(qb, np.int8)
        m, k = q_in.shape
        n = qw.shape[0]
        di, dw, db = self.put(q_in), self.put(qw), self.put(qb)
        oc = self.empty((n,), np.int32)
        ck(lib().i8ie_linear_offsets(self.h, dw.ptr, n, k, C.c_uint8(zp_in), oc.ptr))
        out = self.empty((m, n), np.uint8)
        acc = self.empty((m, n), np.int32) if want_acc else None
        ck(lib().i8ie_linear_u8s8(self.h, di.ptr, m, k, dw.ptr, db.ptr, n, oc.ptr, C.c_float(s_in), C.c_float(s_w),
                                  C.c_float(s_out), C.c_uint8(zp_out), out.ptr, acc.ptr if acc else None))
        r = (out.get(), acc.get() if acc else None, oc.get())
        for b in (di, dw, db, oc, out, acc):
            if b is not None:
                b.free()
        return r

    def conv2d(self, q_in, qw, qb, stride, pad, s_in, zp_in, s_w, s_out, zp_out, want_acc=True):
        """Stateless i8ie_conv2d_u8s8.  Returns (out NCHW, acc [n, oh*ow, kc] or None, oc)."""
        q_in = np.ascontiguousarray(q_in, np.uint8)
        qw = np.ascontiguousarray(qw, np.int8)
        qb = np.ascontiguousarray(qb, np.int8)
        n, c, h, w = q_in.shape
        kc, _, kh, kw = qw.shape
        oh, ow = (h - kh + 2 * pad) // stride + 1, (w - kw + 2 * pad) // stride + 1
        di, dw, db = self.put(q_in), self.put(qw), self.put(qb)
        oc = self.empty((kc,), np.int32)
        ck(lib().i8ie_conv_offsets(self.h, dw.ptr, db.ptr, kc, c * kh * kw, C.c_float(s_in), C.c_uint8(zp_in), oc.ptr))
        out = self.empty((n, kc, oh, ow), np.uint8)
        acc = self.empty((n, oh * ow, kc), np.int32) if want_acc else None
        ck(lib().i8ie_conv2d_u8s8(self.h, di.ptr, n, c, h, w, dw.ptr, kc, kh, kw, stride, pad, C.c_uint8(zp_in),
                                  oc.ptr, C.c_float(s_in), C.c_float(s_w), C.c_float(s_out), C.c_uint8(zp_out),
                                  out.ptr, acc.ptr if acc else None))
        r = (out.get(), acc.get() if acc else None, oc.get())
        for b in (di, dw, db, oc, out, acc):
            if b is not None:
                b.free()
        return r

    def layer_forward(self, kind, q_in, qw, qb, s_in, zp_in, s_w, s_out, zp_out, stride=1, pad=0, repeat=1,
                      want_acc=True):
        """Through the layer-handle API (i8ie_*_create / set_output_qparams / forward)."""
        q_in = np.ascontiguousarray(q_in, np.uint8)
        qw = np.ascontiguousarray(qw, np.int8)
        qb = np.ascontiguousarray(qb, np.int8)
        L = C.c_void_p()
        if kind == "linear":
            m, k = q_in.shape
            n = qw.shape[0]
            ck(lib().i8ie_linear_create(self.h, qw.ctypes.data_as(C.c_void_p), qb.ctypes.data_as(C.c_void_p), n, k,
                                        C.c_float(s_w), C.byref(L)))
            oshape, ashape, h, w = (m, n), (m, n), 0, 0
        else:
            m, c, h, w = q_in.shape
            kc, _, kh, kw = qw.shape
            oh, ow = (h - kh + 2 * pad) // stride + 1, (w - kw + 2 * pad) // stride + 1
            ck(lib().i8ie_conv2d_create(self.h, qw.ctypes.data_as(C.c_void_p), qb.ctypes.data_as(C.c_void_p), kc, c,
                                        kh, kw, stride, pad, C.c_float(s_w), C.byref(L)))
            oshape, ashape = (m, kc, oh, ow), (m, oh * ow, kc)
        ck(lib().i8ie_layer_set_output_qparams(L, C.c_float(s_out), C.c_uint8(zp_out)))
        di = self.put(q_in)
        out = self.empty(oshape, np.uint8)
        acc = self.empty(ashape, np.int32) if want_acc else None
        for _ in range(repeat):
            ck(lib().i8ie_layer_forward(L, di.ptr, m, h, w, C.c_float(s_in), C.c_uint8(zp_in), out.ptr,
                                        acc.ptr if acc else None))
        r = (out.get(), acc.get() if acc else None)
        lib().i8ie_layer_destroy(L)
        for b in (di, out, acc):
            if b is not None:
                b.free()
        return r

    # ---- FP32 ops (include/i8ie_hip.h, "FP32 ops") ------------------------------
    def guarded(self, shape):
        """A float32 output of `shape` inside a larger device buffer (GuardedOut)."""
        return GuardedOut(self, shape)

    def linear_f32(self, x, w, b):
        """i8ie_linear_f32: x [m, k], w [n, k], b [n] -> (out [m, n], guards untouched?)."""
        x, w, b = (np.ascontiguousarray(a, np.float32) for a in (x, w, b))
        (m, k), n = x.shape, w.shape[0]
        assert w.shape == (n, k) and b.shape == (n,)
        di, dw, db, o = self.put(x), self.put(w), self.put(b), self.guarded((m, n))
        try:
            ck(lib().i8ie_linear_f32(self.h, di.ptr, m, k, dw.ptr, db.ptr, n, o.ptr))
            return o.read()
        finally:
            for d in (di, dw, db, o):
                d.free()

    def conv2d_f32(self, x, w, b, stride, pad):
        """i8ie_conv2d_f32: x [n, c, h, w], w [kc, c, kh, kw], b [kc] -> (out [n, kc, oh, ow], guards untouched?)."""
        x, w, b = (np.ascontiguousarray(a, np.float32) for a in (x, w, b))
        n, c, h, wd = x.shape
        kc, c2, kh, kw = w.shape
        assert c2 == c and b.shape == (kc,)
        oh, ow = (h - kh + 2 * pad) // stride + 1, (wd - kw + 2 * pad) // stride + 1
        di, dw, db, o = self.put(x), self.put(w), self.put(b), self.guarded((n, kc, oh, ow))
        try:
            ck(lib().i8ie_conv2d_f32(self.h, di.ptr, n, c, h, wd, dw.ptr, db.ptr, kc, kh, kw, stride, pad, o.ptr))
            return o.read()
        finally:
            for d in (di, dw, db, o):
                d.free()

    def relu_f32(self, x):
        x = np.ascontiguousarray(x, np.float32)
        d, o = self.put(x), self.empty(x.shape, np.float32)
        ck(lib().i8ie_relu_f32(self.h, d.ptr, o.ptr, C.c_int64(x.size)))
        r = o.get()
        d.free(); o.free()
        return r

    def maxpool2d_f32(self, x, k, s):
        x = np.ascontiguousarray(x, np.float32)
        n, c, h, w = x.shape
        oh, ow = (h - k) // s + 1, (w - k) // s + 1
        d, o = self.put(x), self.empty((n, c, oh, ow), np.float32)
        ck(lib().i8ie_maxpool2d_f32(self.h, d.ptr, o.ptr, n, c, h, w, k, s))
        r = o.get()
        d.free(); o.free()
        return r

    # ---- v2 entry points ----------------------------------------------------
    def set_force_fallback(self, on):
        ck(lib().i8ie_ctx_set_option(self.h, 1, 1 if on else 0))

    def layout_convert(self, q, to_nhwc, border=0, fill=0):
        """NCHW numpy -> physical NHWC (with border) numpy, or back."""
        q = np.ascontiguousarray(q, np.uint8)
        if to_nhwc:
            n, c, h, w = q.shape
            oshape = (n, h + 2 * border, w + 2 * border, c)
        else:
            n, hp, wp, c = q.shape
            h, w = hp - 2 * border, wp - 2 * border
            oshape = (n, c, h, w)
        d, o = self.put(q), self.empty(oshape, np.uint8)
        ck(lib().i8ie_layout_convert_u8(self.h, d.ptr, o.ptr, n, c, h, w, 1 if to_nhwc else 0, border, C.c_uint8(fill)))
        r = o.get()
        d.free(); o.free()
        return r

    def max_pool2d_nhwc(self, q_phys, k, s, in_border=0, out_border=0, fill=0):
        q = np.ascontiguousarray(q_phys, np.uint8)
        n, hp, wp, c = q.shape
        h, w = hp - 2 * in_border, wp - 2 * in_border
        oh, ow = (h - k) // s + 1, (w - k) // s + 1
        d, o = self.put(q), self.empty((n, oh + 2 * out_border, ow + 2 * out_border, c), np.uint8)
        ck(lib().i8ie_fill_border_u8(self.h, o.ptr, n, c, oh, ow, out_border, C.c_uint8(fill)))
        ck(lib().i8ie_maxpool2d_u8_nhwc(self.h, d.ptr, in_border, o.ptr, out_border, n, c, h, w, k, s))
        r = o.get()
        d.free(); o.free()
        return r

    def set_variant(self, value):
        ck(lib().i8ie_ctx_set_option(self.h, 2, int(value)))

    @contextlib.contextmanager
    def launch_map(self):
        """Inside: every launch on this ctx is profiled.  Yields a dict that holds, once the block has ended, kernel name
        (cut at '|') -> launches."""
        got = {}
        ck(lib().i8ie_profile_start(self.h, 0))
        try:
            yield got
        finally:
            ents, cnt = (ProfEntry * 128)(), C.c_int(0)
            ck(lib().i8ie_profile_stop(self.h, ents, 128, C.byref(cnt)))
            for e in ents[:cnt.value]:
                name = e.name.decode().split("|")[0]
                got[name] = got.get(name, 0) + int(e.launches)

    def kernels_run(self, fn):
        """(fn(), the names -- cut at '|' -- of the kernels that ran on this ctx inside it, one per (kernel, problem size))"""
        ck(lib().i8ie_profile_start(self.h, 0))
        try:
            res = fn()
        finally:
            ents, cnt = (ProfEntry * 64)(), C.c_int(0)
            ck(lib().i8ie_profile_stop(self.h, ents, 64, C.byref(cnt)))
        return res, [e.name.decode().split("|")[0] for e in ents[:cnt.value]]

    def layer_queries(self, L, m, h, w, pool_k, pool_s):
        """The layout / pool negotiation answers of a layer handle at batch m, input h x w, with this pool behind it."""
        fuses, reads, stores, f32, pref = (C.c_int(-1) for _ in range(5))
        ck(lib().i8ie_layer_fuses_pool(L, m, h, w, pool_k, pool_s, C.byref(fuses)))
        ck(lib().i8ie_layer_rebiased_io(L, m, h, w, pool_k, pool_s, C.byref(reads), C.byref(stores)))
        ck(lib().i8ie_layer_accepts_f32_input(L, h, w, C.byref(f32)))
        ck(lib().i8ie_layer_preferred_layout(L, C.byref(pref)))
        return dict(fuses_pool=fuses.value, reads_s8=reads.value, stores_s8=stores.value, accepts_f32=f32.value,
                    preferred_layout=pref.value)

    @staticmethod
    def to_phys(q_nchw, border, fill):
        """host-side NCHW -> bordered NHWC"""
        n, c, h, w = q_nchw.shape
        p = np.full((n, h + 2 * border, w + 2 * border, c), fill, np.uint8)
        p[:, border:border + h, border:border + w, :] = q_nchw.transpose(0, 2, 3, 1)
        return p

    def layer_forward_fused(self, kind, q_in_nchw, qw, qb, s_in, zp_in, s_w, s_out, zp_out, stride=1, pad=0,
                            in_nhwc=False, out_nhwc=False, relu=False, want_acc=True, in_border=0, out_border=0,
                            flat_chw=None):
        """i8ie_layer_forward_fused.  Input is given in NCHW and laid out on the host as asked (NHWC with a
        zero-point border when in_nhwc); the output is returned in NCHW together with the raw physical array.
        Linear with flat_chw=(c, h, w) and in_nhwc: the [m][c*h*w] rows are handed over as flattened NHWC."""
        q_in = np.ascontiguousarray(q_in_nchw, np.uint8)
        qw = np.ascontiguousarray(qw, np.int8)
        qb = np.ascontiguousarray(qb, np.int8)
        L = C.c_void_p()
        if kind == "linear":
            m, k = q_in.shape
            n = qw.shape[0]
            ck(lib().i8ie_linear_create(self.h, qw.ctypes.data_as(C.c_void_p), qb.ctypes.data_as(C.c_void_p), n, k,
                                        C.c_float(s_w), C.byref(L)))
            oshape, ashape, h, w = (m, n), (m, n), 0, 0
            phys_in = q_in
            if flat_chw is not None and in_nhwc:
                cc, h, w = flat_chw
                phys_in = np.ascontiguousarray(q_in.reshape(m, cc, h, w).transpose(0, 2, 3, 1)).reshape(m, k)
        else:
            m, c, h, w = q_in.shape
            kc, _, kh, kw = qw.shape
            oh, ow = (h - kh + 2 * pad) // stride + 1, (w - kw + 2 * pad) // stride + 1
            ck(lib().i8ie_conv2d_create(self.h, qw.ctypes.data_as(C.c_void_p), qb.ctypes.data_as(C.c_void_p), kc, c,
                                        kh, kw, stride, pad, C.c_float(s_w), C.byref(L)))
            ashape = (m, oh * ow, kc)
            oshape = (m, oh + 2 * out_border, ow + 2 * out_border, kc) if out_nhwc else (m, kc, oh, ow)
            phys_in = self.to_phys(q_in, in_border, zp_in) if in_nhwc else q_in
        ck(lib().i8ie_layer_set_output_qparams(L, C.c_float(s_out), C.c_uint8(zp_out)))
        pref = C.c_int(-1)
        ck(lib().i8ie_layer_preferred_layout(L, C.byref(pref)))
        di = self.put(phys_in)
        out = self.empty(oshape, np.uint8)
        acc = self.empty(ashape, np.int32) if want_acc else None
        if kind != "linear" and out_nhwc and out_border:
            ck(lib().i8ie_fill_border_u8(self.h, out.ptr, m, oshape[3], oshape[1] - 2 * out_border,
                                         oshape[2] - 2 * out_border, out_border, C.c_uint8(zp_out)))
        ck(lib().i8ie_layer_forward_fused(L, di.ptr, 1 if in_nhwc else 0, in_border, m, h, w, C.c_float(s_in),
                                          C.c_uint8(zp_in), 1 if relu else 0, out.ptr, 1 if out_nhwc else 0,
                                          out_border, acc.ptr if acc else None))
        phys = out.get()
        o = phys
        if kind != "linear" and out_nhwc:
            b = out_border
            if b:
                ring = phys.copy()
                ring[:, b:-b, b:-b, :] = zp_out
                assert (ring == zp_out).all(), "output border must hold zp_out"
                o = phys[:, b:-b, b:-b, :]
            o = np.ascontiguousarray(o.transpose(0, 3, 1, 2))
        r = (o, acc.get() if acc else None, pref.value)
        lib().i8ie_layer_destroy(L)
        for bb in (di, out, acc):
            if bb is not None:
                bb.free()
        return r

    def layer_forward_pool(self, q_in_nchw, qw, qb, s_in, zp_in, s_w, s_out, zp_out, stride=1, pad=0, in_nhwc=False,
                           out_nhwc=False, relu=False, in_border=0, out_border=0, pool=None, variant=0, in_s8=False,
                           out_s8=False, names=None, guard=None):
        """i8ie_layer_forward_pool (pool=(k, s)) or i8ie_layer_forward_fused (pool=None) of a conv layer.
        in_s8 / out_s8: the NHWC input / output in the re-biased form (I8IE_LAYOUT_NHWC_S8: every byte ^ 0x80, borders
        included).  names: list that receives the kernels that ran.  guard: a dict; when given, the output and the
        accumulators live in GuardedU8 regions and it receives "phys" (the whole physical output as the call left it,
        the re-bias undone) and "ok" (no guard byte of either region changed).
        Returns (out NCHW, acc [n, oh*ow, kc])."""
        q_in = np.ascontiguousarray(q_in_nchw, np.uint8)
        qw = np.ascontiguousarray(qw, np.int8)
        qb = np.ascontiguousarray(qb, np.int8)
        m, c, h, w = q_in.shape
        kc, _, kh, kw = qw.shape
        oh, ow = (h - kh + 2 * pad) // stride + 1, (w - kw + 2 * pad) // stride + 1
        ph, pw = (oh, ow) if pool is None else ((oh - pool[0]) // pool[1] + 1, (ow - pool[0]) // pool[1] + 1)
        L = C.c_void_p()
        ck(lib().i8ie_conv2d_create(self.h, qw.ctypes.data_as(C.c_void_p), qb.ctypes.data_as(C.c_void_p), kc, c, kh, kw,
                                    stride, pad, C.c_float(s_w), C.byref(L)))
        ck(lib().i8ie_layer_set_output_qparams(L, C.c_float(s_out), C.c_uint8(zp_out)))
        assert not (in_s8 and not in_nhwc) and not (out_s8 and not out_nhwc)
        phys_in = self.to_phys(q_in, in_border, zp_in) if in_nhwc else q_in
        if in_s8:
            phys_in = phys_in ^ np.uint8(0x80)
        di = self.put(phys_in)
        oshape = (m, ph + 2 * out_border, pw + 2 * out_border, kc) if out_nhwc else (m, kc, ph, pw)
        if guard is None:
            out = self.empty(oshape, np.uint8)
            acc = self.empty((m, oh * ow, kc), np.int32)
        else:
            out = GuardedU8(self, oshape)
            acc = GuardedU8(self, (m, oh * ow, kc), np.int32)
        ozp = zp_out ^ (0x80 if out_s8 else 0)
        if out_nhwc and out_border:
            ck(lib().i8ie_fill_border_u8(self.h, out.ptr, m, kc, ph, pw, out_border, C.c_uint8(ozp)))
        il = (2 if in_s8 else 1) if in_nhwc else 0
        ol = (2 if out_s8 else 1) if out_nhwc else 0

        ck(lib().i8ie_ctx_set_option(self.h, 2, variant))
        if names is not None:
            ck(lib().i8ie_profile_start(self.h, 0))
        try:
            if pool is None:
                ck(lib().i8ie_layer_forward_fused(L, di.ptr, il, in_border, m, h, w, C.c_float(s_in),
                                                  C.c_uint8(zp_in), 1 if relu else 0, out.ptr, ol,
                                                  out_border, acc.ptr))
            else:
                ck(lib().i8ie_layer_forward_pool(L, di.ptr, il, in_border, m, h, w, C.c_float(s_in),
                                                 C.c_uint8(zp_in), 1 if relu else 0, pool[0], pool[1], out.ptr,
                                                 ol, out_border, acc.ptr))
        finally:
            ck(lib().i8ie_ctx_set_option(self.h, 2, 0))
            if names is not None:
                ents = (ProfEntry * 64)()
                cnt = C.c_int(0)
                ck(lib().i8ie_profile_stop(self.h, ents, 64, C.byref(cnt)))
                names.extend(ents[i].name.decode().split("|")[0] for i in range(cnt.value))
        phys = out.get()
        if out_s8:
            phys = phys ^ np.uint8(0x80)
        o = phys
        if out_nhwc:
            b = out_border
            if b:
                ring = phys.copy()
                ring[:, b:-b, b:-b, :] = zp_out
                assert (ring == zp_out).all(), "output border must hold zp_out"
                o = phys[:, b:-b, b:-b, :]
            o = np.ascontiguousarray(o.transpose(0, 3, 1, 2))
        r = (o, acc.get())
        if guard is not None:
            guard["phys"], guard["ok"] = phys, out.guards_ok() and acc.guards_ok()
        lib().i8ie_layer_destroy(L)
        for bb in (di, out, acc):
            bb.free()
        return r
