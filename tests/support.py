"""What the test files share: the `i8ie` fixture, the factories of the context / library / JSON fixtures, the layer builders
of the Python-surface tests, the launch counting of the binding's profiler, and a few pure helpers.  An ordinary module: a
test file imports what it uses (a fixture by name, `from support import i8ie  # noqa: F401`, or under the name its tests ask
for, `ctx = support.ctx_fixture(ar)`).  The arithmetic restatements stay in the *_ref.py modules."""
import hashlib
import json
import os
import socket

import numpy as np
import pytest

import abi
from conftest import GOLDEN

f32 = np.float32


# ---- fixtures --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def i8ie():
    import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
    import i8ie as mod

    return mod


def ctx_fixture(*ref_modules):
    """A module-scoped fixture: one abi.Ctx on device 0, closed at the module's end, with the entry points of the given
    *_ref modules bound.  pytest names it after the attribute it is assigned to (`ctx = ...`, `gpu = ...`)."""
    @pytest.fixture(scope="module")
    def fixture():
        import int8inferenceengine_amd  # noqa: F401  (torch's HIP runtime first)

        c = abi.Ctx(0)
        for m in ref_modules:
            m.bind(abi.lib())
        yield c
        c.close()

    return fixture


def lib_fixture(ref_module):
    """A module-scoped fixture: the library with the entry points of one *_ref module bound (no context, no GPU)."""
    @pytest.fixture(scope="module")
    def fixture():
        return ref_module.bind(abi.lib())

    return fixture


def load_json(path):
    with open(path) as f:
        return json.load(f)


def golden_json(name):
    return load_json(os.path.join(GOLDEN, name))


def json_fixture(path):
    """A module-scoped fixture: the content of one recorded JSON file."""
    @pytest.fixture(scope="module")
    def fixture():
        return load_json(path)

    return fixture


def byte_pairs():
    """all 65 536 (a, b) byte pairs as two flat arrays"""
    v = np.arange(256, dtype=np.uint8)
    return np.repeat(v, 256), np.tile(v, 256)


@pytest.fixture(scope="module")
def pairs(ctx):
    """byte_pairs() as flat tensors, resident on the device of the importing module's `ctx`, and one output buffer"""
    a, b = byte_pairs()
    da, db, do = ctx.put(a), ctx.put(b), ctx.empty(a.shape, np.uint8)
    yield a, b, da, db, do
    for d in (da, db, do):
        d.free()


# ---- converted layers of the Python surface (the random stream and the call order fix the expected bytes) ---------------------
def conv(i8ie, cin, cout, k, pad, seed, qp, stride=1):
    rng = np.random.default_rng(seed)
    L = i8ie.Conv2d(cin, cout, k, stride=stride, padding=pad)
    L.load_weight((rng.uniform(-1, 1, (cout, cin, k, k)) * np.sqrt(6.0 / (cin * k * k))).astype(f32))
    L.load_bias(rng.uniform(-0.1, 0.1, cout).astype(f32))
    L.set_output_qparams(*qp)
    L.convert()
    return L


def activation(i8ie, hw=8):
    """an activation as it is inside a network: in the engine's layout and still recorded (test_gpu_add.py's construction).
    The warm-up forward launches it once, with the border its consumers ask for, and the counted forward finds that result."""
    xin = np.random.default_rng(4).uniform(-2, 2, (2, 3, hw, hw)).astype(f32)
    return i8ie.relu(conv(i8ie, 16, 16, 3, 1, 8, (0.05, 125))(i8ie.relu(conv(i8ie, 3, 16, 3, 1, 9, (0.05, 128))(
        i8ie.quantize(i8ie.tensor(xin), 0.025, 127)))))


def conv_ref(L, q, s_in, zp_in, pad=0, stride=1):
    """the bytes a converted conv() layer must give on q, by grouped_ref's restatement"""
    import grouped_ref as gr

    s_out, zp_out = L.output_qparams()
    return gr.conv2d_grouped(q, L.layer.q_weight(), L.layer.q_bias(), 1, stride, pad, f32(s_in), zp_in, L.weight_scale(),
                             f32(s_out), zp_out)[0]


NORM_QP = (f32(0.025), f32(0.02), 128, f32(1e-5))   # s_in, s_out, zp_out, eps


def norm_params(ctx, Cn, seed, qp=NORM_QP):
    """(gamma, beta, and the two folded vectors on the device) of a LayerNorm / GroupNorm case; gamma[0] is zero"""
    import layernorm_ref as lr

    rng = np.random.default_rng(seed)
    gamma = rng.normal(1.0, 0.6, Cn).astype(f32)
    beta = rng.normal(0.0, 0.6, Cn).astype(f32)
    gamma[0] = 0.0
    g, b = lr.affine(gamma, beta, qp[1], qp[2])
    return gamma, beta, ctx.put(g), ctx.put(b)


# ---- launch counts of the binding's profiler ---------------------------------------------------------------------------------
GLUE_KERNELS = ("relu_u8", "rebias", "fill_border", "reborder", "layout_")


def launch_counts(prof):
    """{kernel name: launches} of a profile_stop() dict {"name|size": (launches, ...)}: a kernel name comes once per problem
    size, and the sizes are summed"""
    launches = {}
    for k, v in prof.items():
        name = k.split("|")[0]
        launches[name] = launches.get(name, 0) + v[0]
    return launches


def assert_no_glue_launches(launches):
    """no kernel that only converts, re-biases, fills or clamps ran: for the callers whose operator takes all of that into
    its own launch (where such a launch is legitimate, do not call this)"""
    for k in launches:
        assert not k.startswith(GLUE_KERNELS), launches


def split_launches(launches, prefix):
    """(launches of the kernels named prefix*, launches of all others, launches) of launch_counts() in which no glue kernel
    may occur"""
    assert_no_glue_launches(launches)
    own = sum(v for k, v in launches.items() if k.startswith(prefix))
    return own, sum(v for k, v in launches.items() if not k.startswith(prefix)), launches


def _warm_then_profile(make):
    """make() returns the tensors to launch.  One warm-up call (packs weights, fills cached borders), observed; then a second
    call with every launch profiled.  Returns (the warm-up's arrays, the second call's tensors, {name: launches})."""
    import _CXX_i8ie as cx

    first = [t.numpy() for t in make()]
    cx.synchronize()
    cx.profile_start()
    try:
        again = make()
        for t in again:
            t.data.layout()  # launches what is pending; the bytes are observed outside the counted region
    finally:
        prof = cx.profile_stop()
    return first, again, launch_counts(prof)


def counted(make):
    """{kernel name: launches} of make() -- a function that returns the tensors to launch -- after one warm-up call"""
    return _warm_then_profile(make)[2]


def counted_forward(forward):
    """counted() of a forward with one result: (the warm-up's output, the counted call's output, {name: launches})"""
    first, again, launches = _warm_then_profile(lambda: [forward()])
    print(launches)
    return first[0], again[0].numpy(), launches


# ---- pure helpers ----------------------------------------------------------------------------------------------------------
def phys_nhwc(x_nchw, border, fill, s8):
    """[n, c, h, w] u8 -> the physical buffer [n, h+2b, w+2b, c] with `fill` in the border (all of it re-biased if s8)"""
    n, c, h, w = x_nchw.shape
    p = np.full((n, h + 2 * border, w + 2 * border, c), fill, np.uint8)
    p[:, border:border + h, border:border + w, :] = x_nchw.transpose(0, 2, 3, 1)
    return p ^ np.uint8(0x80) if s8 else p


def byte_image(c):
    """[1, c, 16, 16]: pixel p holds byte p in every channel"""
    return np.broadcast_to(np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16), (1, c, 16, 16)).copy()


def nhwc(x_nchw):
    return np.ascontiguousarray(x_nchw.transpose(0, 2, 3, 1))


def same_bits(got, want):
    """two float32 (or two uint32) arrays of one shape with the same bit patterns"""
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def bits_equal(a, b):
    """same_bits() of anything that converts to float32 (for the strict form that also asks for the dtype: test_gpu_fp32.py)"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def rand_qkv(rng, b, tq, tk, c):
    return (rng.integers(0, 256, (b, tq, c), dtype=np.uint8), rng.integers(0, 256, (b, tk, c), dtype=np.uint8),
            rng.integers(0, 256, (b, tk, c), dtype=np.uint8))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]
