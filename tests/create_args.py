"""The argument rules of the layer-creating entries of the C-ABI, as a table: the ten create entries, the three stateless
entries that build a temporary handle and i8ie_conv2d_u8s8, each called with a NULL ctx (every rule answers before any
device call; the all-valid tuple is refused for its ctx) over a grid of argument tuples.  tests/golden/create_arg_rules.json
is that table as tests/golden/make_create_arg_rules.py recorded it; tests/test_create_args_host.py replays it.

A signature is the entry's C parameter list as tokens: an int parameter by its name, and
    ctx      always NULL                         qw, qb   host weights / bias (never read before the ctx is refused)
    dev      a device pointer (in, qw, oc, out)  acc      always NULL (optional in the ABI)
    s_w      a per-tensor scale                  scales   float[kc]: the `scales` tag of the row
    f, u8    a float / uint8_t quantisation parameter
    out      i8ie_layer**
The `ptrs` tag of a row nulls pointers: "ok" none, "out" the handle's address, "data" every qw / qb / dev."""
import ctypes as C
import itertools

import numpy as np

_CREATE_TAIL = {False: ("s_w", "out"), True: ("scales", "out")}
_IO = ("u8", "dev", "f", "s_w", "f", "u8", "dev", "acc")  # zp_in, oc, s_in, s_w, s_out, zp_out, out, acc


def _create(ints, pc):
    return ("ctx", "qw", "qb") + ints + _CREATE_TAIL[pc]


_CONV = ("kc", "c", "kh", "kw", "stride", "pad")
_DECONV = ("kc", "c", "k", "stride", "pad", "output_pad")
SIGNATURES = {
    "i8ie_linear_create": _create(("n", "k"), False),
    "i8ie_linear_create_per_channel": _create(("n", "k"), True),
    "i8ie_conv2d_create": _create(_CONV, False),
    "i8ie_conv2d_create_per_channel": _create(_CONV, True),
    "i8ie_conv2d_create_grouped": _create(_CONV + ("groups",), False),
    "i8ie_conv2d_create_grouped_per_channel": _create(_CONV + ("groups",), True),
    "i8ie_conv2d_create_dilated": _create(_CONV + ("groups", "dilation"), False),
    "i8ie_conv2d_create_dilated_per_channel": _create(_CONV + ("groups", "dilation"), True),
    "i8ie_conv_transpose2d_create": _create(_DECONV, False),
    "i8ie_conv_transpose2d_create_per_channel": _create(_DECONV, True),
    "i8ie_conv2d_u8s8": ("ctx", "dev", "n", "c", "h", "w", "dev") + _CONV[:1] + _CONV[2:] + _IO,
    "i8ie_conv2d_u8s8_grouped": ("ctx", "dev", "n", "c", "h", "w", "dev") + _CONV[:1] + _CONV[2:] + ("groups",) + _IO,
    "i8ie_conv2d_u8s8_dilated": ("ctx", "dev", "n", "c", "h", "w", "dev") + _CONV[:1] + _CONV[2:] + ("groups", "dilation") + _IO,
    "i8ie_conv_transpose2d_u8s8": ("ctx", "dev", "n", "c", "h", "w", "dev") + _DECONV[:1] + _DECONV[2:] + _IO,
}
_TOKENS = {"ctx", "qw", "qb", "dev", "acc", "s_w", "scales", "f", "u8", "out"}


def int_params(entry):
    return [t for t in SIGNATURES[entry] if t not in _TOKENS]


# ---- the grid --------------------------------------------------------------------------------------------------------
# per parameter: a non-positive value, ordinary values and the boundary values of the entries that take it.  kc / c = 6 is
# not divisible by groups = 4; 65536 groups divide 65536 channels (the bound on groups itself); pad = 3 is the kernel size
# (one past the transposed rule); output_pad = 2 is the ordinary stride; h = w = 1 is smaller than the kernel.
VALUES = {
    "n": (0, 2), "k": (0, -3, 24), "kc": (0, -4, 4, 6, 65536), "c": (0, 4, 6, 65536), "kh": (0, 1, 3), "kw": (0, 1, 3),
    "stride": (0, 1, 2), "pad": (-1, 0, 1, 3), "groups": (0, 1, 2, 4, 65536), "dilation": (0, 1, 2),
    "output_pad": (-1, 0, 2), "h": (0, 1, 8), "w": (0, 1, 8),
}  # ("k" is Linear's in_features; the transposed entries' kernel size and stride take KERNEL and DECONV_STRIDE)
KERNEL = (0, 1, 3, 128, 65536)  # (65536 channels x 128 x 128 is the reduction-length bound)
DECONV_STRIDE = (0, 1, 2, 65536)
# every base tuple is valid; single replaced values are taken around each, pairs of them around the first
BASES = {
    "linear": [dict(n=4, k=24)],
    "conv": [dict(n=2, h=8, w=8, kc=4, c=4, kh=3, kw=3, stride=2, pad=1, groups=2, dilation=2),
             dict(n=2, h=8, w=8, kc=4, c=4, kh=3, kw=3, stride=1, pad=0, groups=1, dilation=1),
             dict(n=2, h=8, w=8, kc=4, c=4, kh=1, kw=1, stride=1, pad=0, groups=2, dilation=2)],
    "deconv": [dict(n=2, h=8, w=8, kc=4, c=4, k=3, stride=2, pad=1, output_pad=1)],
}
SCALES = ("ok", "negative", "nan", "null")
PTRS = ("ok", "out", "data")  # ("out": the create entries only)


def _kind(entry):
    return "linear" if "linear" in entry else "deconv" if "transpose" in entry else "conv"


def _values(entry, p):
    if _kind(entry) == "deconv" and p in ("k", "stride"):
        return KERNEL if p == "k" else DECONV_STRIDE
    return VALUES[p]


def grid(entry):
    """the rows of one entry: (ints in int_params order, scales tag, ptrs tag), without repeats, in a fixed order"""
    names = int_params(entry)
    pc = "scales" in SIGNATURES[entry]
    rows, seen = [], set()

    def add(d, scales="ok", ptrs="ok"):
        r = (tuple(d[p] for p in names), scales if pc else "ok", ptrs)
        if r not in seen:
            seen.add(r)
            rows.append(r)

    for i, base in enumerate(BASES[_kind(entry)]):
        add(base)
        for p in names:
            for v in _values(entry, p):
                add(dict(base, **{p: v}))
        for p, q in itertools.combinations(names, 2) if i == 0 else ():
            for v in _values(entry, p):
                for u in _values(entry, q):
                    add(dict(base, **{p: v, q: u}))
        if "groups" in names:  # the bound on groups itself needs both channel counts to be multiples of it
            for g in (65535, 65536):
                add(dict(base, kc=2 * g, c=g, groups=g))
        # a rule on the scales or a null pointer together with nothing else wrong, and with one more violation
        first = names[0]
        for d in (base, dict(base, **{first: 0}), dict(base, pad=-1) if "pad" in names else base,
                  dict(base, groups=3) if "groups" in names else base, dict(base, dilation=0) if "dilation" in names else base,
                  dict(base, output_pad=2) if "output_pad" in names else base):
            for s in SCALES if pc else ("ok",):
                for ptrs in PTRS if "out" in SIGNATURES[entry] else ("ok", "data"):
                    add(d, s, ptrs)
    return rows


# ---- one call ----------------------------------------------------------------------------------------------------------
_DUMMY = np.zeros(64, np.int8)


def call(lib, entry, ints, scales="ok", ptrs="ok"):
    """-> (return code, i8ie_last_error() text) of `entry` with a NULL ctx"""
    vals = dict(zip(int_params(entry), ints))
    data = None if ptrs == "data" else _DUMMY.ctypes.data_as(C.c_void_p)
    handle = C.c_void_p()
    n_out = vals.get("kc", vals.get("n", 0))
    sw = np.full(max(int(n_out), 1), 0.5, np.float32)
    if scales == "negative":
        sw[len(sw) // 2] = -0.5
    elif scales == "nan":
        sw[-1] = np.nan
    args = []
    for t in SIGNATURES[entry]:
        if t in ("ctx", "acc"):
            args.append(None)
        elif t in ("qw", "qb", "dev"):
            args.append(data)
        elif t in ("s_w", "f"):
            args.append(C.c_float(0.5))
        elif t == "u8":
            args.append(C.c_uint8(3))
        elif t == "scales":
            args.append(None if scales == "null" else sw.ctypes.data_as(C.c_void_p))
        elif t == "out":
            args.append(None if ptrs == "out" else C.byref(handle))
        else:
            args.append(C.c_int(vals[t]))
    fn = getattr(lib, entry)
    fn.restype = C.c_int
    rc = fn(*args)
    assert handle.value is None, "%s made a handle without a ctx" % entry
    return int(rc), lib.i8ie_last_error().decode()
