"""Position embedding with a class token on the GPU (csrc/i8ie_posembed.hip).  Every comparison of bytes is
exact and against the numpy restatement (tests/posembed_ref.py), never against the code under test; a failure prints the first
differing index."""
import ctypes as C
import itertools

import numpy as np
import pytest

import abi
import int8inferenceengine_amd  # noqa: F401  (puts the i8ie package on the path)
import posembed_ref as pr
import support
from support import i8ie  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32

ctx = support.ctx_fixture(pr)

SENTINEL = 0x3C  # what the result's border holds before the call
POISON = 0xEE    # what the input's border holds: never read


def _first_diff(got, want):
    bad = np.argwhere(got != want)
    return None if bad.size == 0 else (tuple(int(v) for v in bad[0]), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]), len(bad))


def _run(ctx, q, E, cls, qp, relu=False, ib=0, ix=0, ob=0, ox=0, off=0, force=False):
    """i8ie_posembed_u8_nhwc on q [n, c, h, w]: (every byte of the physical result, the bytes expected there, guards untouched?,
    the kernels that ran).  off: the input and the result lie `off` bytes past an aligned address."""
    n, c, h, w = q.shape
    s_in, zp_in, s_out, zp_out = qp
    src = support.phys_nhwc(q, ib, POISON ^ (0x80 if ix else 0), ix)
    dev = ctx.put(np.concatenate([np.zeros(off, np.uint8), src.ravel()]))
    oshape = (n, c, 1, h * w + 1) if cls else (n, c, h, w)
    start = support.phys_nhwc(np.full(oshape, 0xC3, np.uint8), ob, SENTINEL, False)
    out = abi.GuardedU8(ctx, (start.size + off,), fill=np.concatenate([np.full(off, 0xC3, np.uint8), start.ravel()]))
    dE = ctx.put(np.ascontiguousarray(E, f32))
    try:
        ctx.set_force_fallback(force)
        rc, names = ctx.kernels_run(lambda: abi.lib().i8ie_posembed_u8_nhwc(
            ctx.h, C.c_void_p(dev.ptr.value + off), ib, ix, C.c_void_p(out.ptr.value + off), ob, ox, n, c, h, w, 1 if cls else 0, dE.ptr,
            float(s_in), int(zp_in), float(s_out), int(zp_out), 1 if relu else 0))
        abi.ck(rc)
        got = out.get()
        ok = out.guards_ok() and bool((got[:off] == 0xC3).all())
        assert np.array_equal(dev.get()[off:], src.ravel()), "the input was written"
    finally:
        ctx.set_force_fallback(False)
        for d in (dev, out, dE):
            d.free()
    want = start.copy()
    inner = pr.posembed_u8(q, E, cls, s_in, zp_in, s_out, zp_out, relu).transpose(0, 2, 3, 1)
    want[:, ob:ob + inner.shape[1], ob:ob + inner.shape[2], :] = inner ^ np.uint8(0x80) if ox else inner
    return got[off:].reshape(want.shape), want, ok, names


def _bytes_input(n, c, h, w, seed):
    """[n, c, h, w] in which each of the 256 bytes stands at every channel position (so at every position of a lane's item):
    channel ch of flat pixel p holds byte (p + 37 * ch + seed) % 256 where the map has 256 pixels over the batch, random bytes
    beyond"""
    pix = n * h * w
    if pix >= 256:
        p = np.arange(pix).reshape(n, 1, h, w)
        return ((p + 37 * np.arange(c).reshape(1, c, 1, 1) + seed) % 256).astype(np.uint8)
    return np.random.default_rng(seed).integers(0, 256, (n, c, h, w), dtype=np.uint8)


# ---- exhaustive arithmetic ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def all_bytes():
    """every byte at every position of an item of 16, 4 and 1 channels: [256 // 4, c, 2, 2] holds byte (p + 37 ch) % 256"""
    return {c: _bytes_input(64, c, 2, 2, 0) for c in (16, 48, 20, 3, 35)}


@pytest.mark.parametrize("cls", [False, True], ids=["plain", "class"])
@pytest.mark.parametrize("name", sorted(pr.SETS))
def test_exhaustive_bytes_both_kernels(ctx, all_bytes, name, cls):
    qp = pr.SETS[name][:4]
    for c, q in all_bytes.items():
        assert all(len(np.unique(q[:, ch])) == 256 for ch in range(c))
        P, tok = pr.make_table(name, 4 + cls, c, cls)
        E = pr.table(P, tok)
        for force, relu in ((False, False), (False, True), (True, False)):
            got, want, ok, names = _run(ctx, q, E, cls, qp, relu=relu, force=force)
            assert names == ["posembed_u8_direct" if force else "posembed_u8_nhwc"], names
            assert ok and _first_diff(got, want) is None, (name, c, force, relu, _first_diff(got, want))


@pytest.mark.parametrize("name", sorted(pr.SETS))
@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (8, 8)])
@pytest.mark.parametrize("n", [1, pr.WALK - 1, pr.WALK + 1])
def test_shapes_and_the_image_loops_tail_and_wrap(ctx, hw, n, name):
    """every parameter set on every map size, below and above the number of images a lane walks (the bytes are random where the
    batch has fewer than 256 pixels: all 256 bytes at every item position is test_exhaustive_bytes_both_kernels' part)"""
    qp = pr.SETS[name][:4]
    for c, cls in itertools.product((16, 48, 20, 3, 35), (False, True)):
        q = _bytes_input(n, c, hw[0], hw[1], c)
        P, tok = pr.make_table(name, hw[0] * hw[1] + cls, c, cls, seed=n)
        for force in (False, True):
            got, want, ok, _ = _run(ctx, q, pr.table(P, tok), cls, qp, force=force)
            assert ok and _first_diff(got, want) is None, (name, hw, n, c, cls, force, _first_diff(got, want))


# ---- layouts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [16, 20])
@pytest.mark.parametrize("cls", [False, True], ids=["plain", "class"])
def test_layout_matrix(ctx, c, cls):
    """input border 0 / 1 / 2, plain / re-biased, times result border 0 / 1, plain / re-biased: only the interior of the result
    changes (its border stays as it was, the guard bands too), and the input's poisoned border is never read"""
    qp = pr.SETS["ordinary"][:4]
    q = np.random.default_rng(c).integers(0, 256, (3, c, 3, 5), dtype=np.uint8)
    P, tok = pr.make_table("ordinary", 15 + cls, c, cls)
    E = pr.table(P, tok)
    for ib, ix, ob, ox in itertools.product((0, 1, 2), (0, 1), (0, 1), (0, 1)):
        got, want, ok, names = _run(ctx, q, E, cls, qp, relu=bool(ib == 1), ib=ib, ix=ix, ob=ob, ox=ox)
        assert names == ["posembed_u8_nhwc"] and ok and _first_diff(got, want) is None, (c, cls, ib, ix, ob, ox, _first_diff(got, want))


def test_result_border_as_fill_border_made_it(ctx):
    """the class form into a bordered re-biased result whose border i8ie_fill_border_u8 made: the border survives the launch"""
    qp = pr.SETS["ordinary"][:4]
    n, c, h, w, ob = 2, 16, 2, 2, 1
    q = np.random.default_rng(1).integers(0, 256, (n, c, h, w), dtype=np.uint8)
    P, tok = pr.make_table("ordinary", 5, c, True)
    E = pr.table(P, tok)
    dev, dE = ctx.put(support.nhwc(q)), ctx.put(E)
    out = abi.GuardedU8(ctx, (n, 1 + 2 * ob, 5 + 2 * ob, c))
    try:
        abi.ck(abi.lib().i8ie_fill_border_u8(ctx.h, out.ptr, n, c, 1, 5, ob, C.c_uint8(qp[3] ^ 0x80)))
        abi.ck(abi.lib().i8ie_posembed_u8_nhwc(ctx.h, dev.ptr, 0, 0, out.ptr, ob, 1, n, c, h, w, 1, dE.ptr, float(qp[0]), qp[1], float(qp[2]), qp[3], 0))
        got, ok = out.get() ^ np.uint8(0x80), out.guards_ok()
    finally:
        for d in (dev, dE, out):
            d.free()
    want = support.phys_nhwc(pr.posembed_u8(q, E, True, *qp), ob, qp[3], False)
    assert ok and _first_diff(got, want) is None, _first_diff(got, want)


# ---- grid and fallbacks --------------------------------------------------------------------------------------------------------------
def test_a_grid_that_wraps(ctx):
    """c = 16 is one item per token and 256 tokens per block: the two tokens of a 1 x 1 class form make one tile, so the units are
    the image groups alone, and MAX_BLOCKS * WALK + 3 images make one more unit than the grid has blocks"""
    qp = pr.SETS["ordinary"][:4]
    n = pr.MAX_BLOCKS * pr.WALK + 3
    q = np.random.default_rng(2).integers(0, 256, (n, 16, 1, 1), dtype=np.uint8)
    P, tok = pr.make_table("ordinary", 2, 16, True)
    got, want, ok, names = _run(ctx, q, pr.table(P, tok), True, qp)
    assert names == ["posembed_u8_nhwc"] and ok and _first_diff(got, want) is None, _first_diff(got, want)


@pytest.mark.parametrize("walk", [8, 4, 2])
def test_every_walk_length_and_its_tail(ctx, walk):
    """a 1 x 1 map is one tile and one channel chunk, so the units are the image groups: FULL_GRID * walk + 1 images keep the walk at
    `walk` (one walk longer would leave fewer than FULL_GRID units) and end in a group of one image"""
    qp = pr.SETS["saturating"][:4]
    n = pr.FULL_GRID * walk + 1
    for c, cls in ((16, True), (20, False), (3, True)):
        q = np.random.default_rng(walk + c).integers(0, 256, (n, c, 1, 1), dtype=np.uint8)
        P, tok = pr.make_table("saturating", 1 + cls, c, cls)
        got, want, ok, names = _run(ctx, q, pr.table(P, tok), cls, qp, relu=True)
        assert names == ["posembed_u8_nhwc"] and ok and _first_diff(got, want) is None, (walk, c, cls, _first_diff(got, want))


@pytest.mark.parametrize("cls", [False, True], ids=["plain", "class"])
def test_unaligned_buffers_take_the_direct_kernel(ctx, cls):
    qp = pr.SETS["saturating"][:4]
    q = np.random.default_rng(3).integers(0, 256, (pr.WALK + 1, 16, 2, 3), dtype=np.uint8)
    P, tok = pr.make_table("saturating", 6 + cls, 16, cls)
    for off in (1, 4):
        got, want, ok, names = _run(ctx, q, pr.table(P, tok), cls, qp, off=off, ib=1, ob=1, ox=1)
        assert names == ["posembed_u8_direct"] and ok and _first_diff(got, want) is None, (off, _first_diff(got, want))


# ---- the FP32 entry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [False, True], ids=["plain", "class"])
def test_fp32_entry_bit_for_bit(ctx, cls):
    rng = np.random.default_rng(4)
    n, c, h, w = 3, 5, 2, 3
    x = rng.normal(0, 2, (n, c, h, w)).astype(f32)
    E = pr.table(rng.normal(0, 1, (h * w + cls, c)).astype(f32), rng.normal(0, 1, c).astype(f32) if cls else None)
    want = pr.posembed_f32(x, E, cls)
    dev, dE, out = ctx.put(x), ctx.put(E), abi.GuardedOut(ctx, want.shape)
    try:
        abi.ck(abi.lib().i8ie_posembed_f32(ctx.h, dev.ptr, out.ptr, n, c, h, w, 1 if cls else 0, dE.ptr))
        got, ok = out.read()
    finally:
        for d in (dev, dE, out):
            d.free()
    assert ok and abi.GuardedOut.unwritten(got) == 0
    assert _first_diff(got.view(np.uint32), want.view(np.uint32)) is None, _first_diff(got.view(np.uint32), want.view(np.uint32))


# ---- the Python surface ------------------------------------------------------------------------------------------------------------
QP_CONV = (0.05, 128)


def _pe(i8ie, c, h, w, cls, qp=(0.04, 120), seed=0):
    P, tok = pr.make_table("ordinary", h * w + cls, c, cls, seed)
    L = i8ie.PositionEmbedding(c, h, w, class_token=cls)
    L.load_weight(P)
    if cls:
        L.load_bias(tok)
    L.set_output_qparams(*qp)
    L.convert()
    return L, pr.table(P, tok)


def _engine_activation(i8ie, n, h, w, seed):
    """(a tensor, its bytes): a relu'd conv result of 16 channels as it is inside a network, launched, in the engine's NHWC layout"""
    stem0 = support.conv(i8ie, 3, 16, 3, 1, 9, (0.05, 128))
    stem1 = support.conv(i8ie, 16, 16, 3, 1, 11, QP_CONV)
    xin = np.random.default_rng(seed).uniform(-3, 3, (n, 3, h, w)).astype(f32)

    def make():
        return i8ie.relu(stem1(i8ie.relu(stem0(i8ie.quantize(i8ie.tensor(xin), 0.025, 127)))))

    return make(), make().numpy()  # (observing a tensor brings its storage to the reference's order: the bytes come from a twin)


@pytest.mark.parametrize("cls", [False, True], ids=["plain", "class"])
def test_launch_counts_conv_posembed_relu_conv(i8ie, cls):
    """conv -> PositionEmbedding -> relu -> conv is three launches: the embedding reads the conv's NHWC result as it lies, takes the
    relu in and writes what the next conv asks for; nothing converts a layout, re-biases or fills a border in between"""
    x, _ = _engine_activation(i8ie, 3, 4, 4, 90)
    stem = support.conv(i8ie, 16, 16, 3, 1, 1, QP_CONV)
    pe, E = _pe(i8ie, 16, 4, 4, cls)
    tail = support.conv(i8ie, 16, 16, 1, 0, 8, (0.05, 125))
    own, others, launches = support.split_launches(support.counted(lambda: [tail(i8ie.relu(pe(stem(x))))]), "posembed_u8")
    assert launches.get("posembed_u8_nhwc") == 1 and (own, others) == (1, 2), launches
    a = stem(x).numpy()
    mid = pr.posembed_u8(a, E, cls, f32(QP_CONV[0]), QP_CONV[1], f32(0.04), 120, relu=True)
    got, want = tail(i8ie.relu(pe(stem(x)))).numpy(), support.conv_ref(tail, mid, 0.04, 120)
    assert _first_diff(got, want) is None, _first_diff(got, want)


def test_launch_counts_posembed_feeding_layernorm_and_add(i8ie):
    """a PositionEmbedding read by a LayerNorm and by an Add skip adds one launch, and both read its result as it lies"""
    import add_ref
    import layernorm_ref as lr

    x, a = _engine_activation(i8ie, 3, 4, 4, 91)
    pe, E = _pe(i8ie, 16, 4, 4, True)
    ln = i8ie.LayerNorm(16)
    ln.set_output_qparams(0.02, 128)
    ln.convert()
    add = i8ie.Add()
    add.set_output_qparams(0.05, 126)
    add.convert()

    def forward():
        t = pe(x)
        return [add(t, ln(t))]

    own, others, launches = support.split_launches(support.counted(forward), "posembed_u8")
    assert launches.get("posembed_u8_nhwc") == 1 and (own, others) == (1, 2), launches  # (the embedding; the LayerNorm and the Add)
    t = pr.posembed_u8(a, E, True, f32(QP_CONV[0]), QP_CONV[1], f32(0.04), 120)
    n_ = lr.layer_norm_u8_nchw(t, f32(0.04), f32(1e-5), np.ones(16, f32), np.zeros(16, f32), f32(0.02), 128)
    want = add_ref.add_u8(t, 120, f32(0.04), n_, 128, f32(0.02), f32(0.05), 126)
    got = forward()[0].numpy()
    assert _first_diff(got, want) is None, _first_diff(got, want)


@pytest.mark.parametrize("method", ["reservoir", "minmax"])
def test_prepare_convert_state_dict_and_graph_replay(i8ie, method, tmp_path):
    from int8inferenceengine_amd import graph

    class Net(i8ie.Module):
        def __init__(self):
            super().__init__()
            self.conv = i8ie.Conv2d(3, 16, 4, stride=4)
            self.pos = i8ie.PositionEmbedding(16, 2, 2, class_token=True)
            self.plain = i8ie.PositionEmbedding(16, 1, 5)
            self.act = i8ie.Activation("hardswish")

        def forward(self, x):
            return self.act(self.plain(self.pos(self.conv(x))))

    rng = np.random.default_rng(6)
    sd = {"conv.weight": rng.normal(0, 0.2, (16, 3, 4, 4)).astype(f32), "conv.bias": rng.normal(0, 0.1, 16).astype(f32),
          "pos.weight": rng.normal(0, 1, (5, 16)).astype(f32), "pos.bias": rng.normal(0, 1, 16).astype(f32),
          "plain.weight": rng.normal(0, 1, (5, 16)).astype(f32)}
    x = rng.uniform(-2, 2, (5, 3, 8, 8)).astype(f32)
    i8ie.set_calibration(method)
    try:
        net = Net()
        net.load(sd)
        net.prepare()
        y32 = net(i8ie.tensor(x)).numpy()
        net.convert()
    finally:
        i8ie.set_calibration("reservoir")
    assert y32.shape == (5, 16, 1, 5)
    for name in ("pos", "plain"):
        s, zp = getattr(net, name).output_qparams()
        assert (s, zp) != (1.0, 0) and 0 < s < 1, (name, s, zp)  # set from the calibration batch
    got = net(i8ie.tensor(x)).numpy()
    state = net.quantized_state_dict()
    assert sorted(k for k in state if k.startswith(("pos", "plain"))) == ["plain.qparams", "plain.weight", "pos.bias", "pos.qparams", "pos.weight"]
    again = Net()
    again.load_quantized(state)
    assert np.array_equal(again(i8ie.tensor(x)).numpy().view(np.uint32), got.view(np.uint32))
    path = str(tmp_path / "pe.npz")
    net.save_quantized(path)
    third = Net()
    third.load_quantized_file(path)
    assert np.array_equal(third(i8ie.tensor(x)).numpy().view(np.uint32), got.view(np.uint32))
    g = graph.GraphedForward(net, i8ie.tensor(x).prefetch())
    for _ in range(2):
        assert np.array_equal(g().numpy().view(np.uint32), got.view(np.uint32))


def test_functional_form_and_the_class_column_into_linear(i8ie):
    """i8ie.position_embedding on uint8 and FP32 tensors, and crop(x, 0, 0, 1, 1).reshape(-1, c) of its result into a Linear"""
    rng = np.random.default_rng(7)
    x = rng.uniform(-6, 6, (5, 16, 2, 2)).astype(f32)
    q = i8ie.quantize(i8ie.tensor(x), 0.05, 128).numpy()  # (the bytes the op below reads: a twin of its operand)
    P, tok = pr.make_table("ordinary", 5, 16, True)
    E = pr.table(P, tok)
    y32 = i8ie.position_embedding(i8ie.tensor(x), P, tok).numpy()
    assert support.same_bits(y32, pr.posembed_f32(x, E, True))
    t = i8ie.position_embedding(i8ie.quantize(i8ie.tensor(x), 0.05, 128), P, tok, scale=0.04, zero_point=120)
    want = pr.posembed_u8(q, E, True, f32(0.05), 128, f32(0.04), 120)
    assert t.shape == (5, 16, 1, 5) and _first_diff(t.numpy(), want) is None
    with pytest.raises(TypeError, match="needs the result's scale"):
        i8ie.position_embedding(t, P[:4])
    with pytest.raises(RuntimeError, match="weight must be float32"):
        i8ie.position_embedding(t, P[:4], scale=0.04, zero_point=120)  # (five tokens, four rows)
    fc = i8ie.Linear(16, 5)
    fc.load_weight(rng.normal(0, 0.3, (5, 16)).astype(f32))
    fc.load_bias(rng.normal(0, 0.1, 5).astype(f32))
    fc.set_output_qparams(0.1, 100)
    fc.convert()
    col = i8ie.crop(t, 0, 0, 1, 1).reshape(-1, 16)
    assert _first_diff(col.numpy(), want[:, :, 0, 0]) is None
    import grouped_ref

    got = fc(i8ie.crop(t, 0, 0, 1, 1).reshape(-1, 16)).numpy()
    ref = grouped_ref.conv2d_grouped(want[:, :, :1, :1], fc.layer.q_weight().reshape(5, 16, 1, 1), fc.layer.q_bias(), 1, 1, 0, f32(0.04), 120,
                                     fc.weight_scale(), f32(0.1), 100)[0].reshape(5, 5)
    assert _first_diff(got, ref) is None, _first_diff(got, ref)


# ---- an encoder block, step by step ------------------------------------------------------------------------------------------------
def _dense(i8ie, kind, cin, cout, k, stride, seed, qp, per_channel):
    """a converted Conv2d (kind "conv") or Linear with seeded weights and the given output (scale, zero_point)"""
    rng = np.random.default_rng(seed)
    shape = (cout, cin, k, k) if kind == "conv" else (cout, cin)
    L = i8ie.Conv2d(cin, cout, k, stride=stride) if kind == "conv" else i8ie.Linear(cin, cout)
    L.load_weight((rng.uniform(-1, 1, shape) * np.sqrt(6.0 / (cin * k * k))).astype(f32))
    L.load_bias(rng.uniform(-0.1, 0.1, cout).astype(f32))
    L.set_output_qparams(*qp)
    L.convert(per_channel)
    return L


def _dense_ref(L, q, s_in, zp_in, stride, per_channel):
    """the bytes a _dense layer must give on q [n, c, h, w] (a Linear: h = w = 1), by the oracle's conv through grouped_ref"""
    import grouped_ref

    s_out, zp_out = L.output_qparams()
    qw = L.layer.q_weight()
    qw = qw.reshape(qw.shape[0], qw.shape[1], 1, 1) if qw.ndim == 2 else qw
    if per_channel:
        return grouped_ref.conv2d_grouped_pc(q, qw, L.layer.q_bias(), 1, stride, 0, f32(s_in), zp_in, L.weight_scales(), f32(s_out), zp_out)[0]
    return grouped_ref.conv2d_grouped(q, qw, L.layer.q_bias(), 1, stride, 0, f32(s_in), zp_in, L.weight_scale(), f32(s_out), zp_out)[0]


@pytest.mark.parametrize("per_channel", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("batch", [1, 5])
def test_encoder_block_step_by_step(i8ie, batch, per_channel):
    """patch conv 3 -> 16 (4x4 stride 4 on 3 x 8 x 8: 4 tokens); PositionEmbedding(16, 2, 2, class_token=True); LN; qkv 1x1;
    Attention(2); proj; Add; LN; 1x1 16 -> 32; hardswish (the engine has no GELU); 1x1 32 -> 16; Add; LN; crop of the class column;
    Linear(16, 5).  Every step's device result against the existing references applied to the previous step's device bytes, eager
    and under the force-fallback option, and the result of a run in which nothing but the output is observed."""
    import _CXX_i8ie as cx
    import act_ref
    import add_ref
    import layernorm_ref as lr
    import mha_ref

    rng = np.random.default_rng(50)
    pc = per_channel
    qp = {"patch": (0.05, 128), "pos": (0.05, 126), "ln1": (0.02, 128), "qkv": (0.03, 127), "attn": (0.03, 128), "proj": (0.04, 125),
          "add1": (0.06, 128), "ln2": (0.02, 130), "fc1": (0.03, 128), "act": (0.02, 20), "fc2": (0.04, 124), "add2": (0.07, 128),
          "ln3": (0.02, 128), "head": (0.05, 128)}
    score_qp = (0.02, 128)
    patch = _dense(i8ie, "conv", 3, 16, 4, 4, 51, qp["patch"], pc)
    P, tok = rng.normal(0, 0.5, (5, 16)).astype(f32), rng.normal(0, 0.5, 16).astype(f32)
    pos = i8ie.PositionEmbedding(16, 2, 2, class_token=True)
    pos.load_weight(P)
    pos.load_bias(tok)
    pos.set_output_qparams(*qp["pos"])
    pos.convert()
    E = pr.table(P, tok)
    norms, affine = {}, {}
    for name in ("ln1", "ln2", "ln3"):
        affine[name] = (rng.normal(1.0, 0.3, 16).astype(f32), rng.normal(0.0, 0.3, 16).astype(f32))
        norms[name] = i8ie.LayerNorm(16)
        norms[name].load_weight(affine[name][0])
        norms[name].load_bias(affine[name][1])
        norms[name].set_output_qparams(*qp[name])
        norms[name].convert()
    qkv = _dense(i8ie, "conv", 16, 48, 1, 1, 52, qp["qkv"], pc)
    attn = i8ie.Attention(2)
    attn.set_score_qparams(*score_qp)
    attn.set_output_qparams(*qp["attn"])
    attn.convert()
    proj = _dense(i8ie, "conv", 16, 16, 1, 1, 53, qp["proj"], pc)
    fc1 = _dense(i8ie, "conv", 16, 32, 1, 1, 54, qp["fc1"], pc)
    fc2 = _dense(i8ie, "conv", 32, 16, 1, 1, 55, qp["fc2"], pc)
    head = _dense(i8ie, "linear", 16, 5, 1, 1, 56, qp["head"], pc)
    act = i8ie.Activation("hardswish")
    act.set_output_qparams(*qp["act"])
    act.convert()
    adds = {}
    for name in ("add1", "add2"):
        adds[name] = i8ie.Add()
        adds[name].set_output_qparams(*qp[name])
        adds[name].convert()
    x = rng.uniform(-2, 2, (batch, 3, 8, 8)).astype(f32)

    def chain():
        t = {}
        t["q0"] = i8ie.quantize(i8ie.tensor(x), 0.025, 127)
        t["patch"] = patch(t["q0"])
        t["pos"] = pos(t["patch"])
        t["ln1"] = norms["ln1"](t["pos"])
        t["qkv"] = qkv(t["ln1"])
        t["attn"] = attn(t["qkv"])
        t["proj"] = proj(t["attn"])
        t["add1"] = adds["add1"](t["pos"], t["proj"])
        t["ln2"] = norms["ln2"](t["add1"])
        t["fc1"] = fc1(t["ln2"])
        t["act"] = act(t["fc1"])
        t["fc2"] = fc2(t["act"])
        t["add2"] = adds["add2"](t["add1"], t["fc2"])
        t["ln3"] = norms["ln3"](t["add2"])
        t["cls"] = i8ie.crop(t["ln3"], 0, 0, 1, 1)
        t["out"] = head(t["cls"].reshape(-1, 16))
        return t

    def s(name):
        return f32(qp[name][0])

    def z(name):
        return qp[name][1]

    def ln_ref(name, q, src):
        return lr.layer_norm_u8_nchw(q, s(src), f32(1e-5), affine[name][0], affine[name][1], s(name), z(name))

    def expected(g):
        """each step's reference on the previous step's device bytes g[...]"""
        w = {}
        w["patch"] = _dense_ref(patch, g["q0"], 0.025, 127, 4, pc)
        w["pos"] = pr.posembed_u8(g["patch"], E, True, s("patch"), z("patch"), s("pos"), z("pos"))
        w["ln1"] = ln_ref("ln1", g["pos"], "pos")
        w["qkv"] = _dense_ref(qkv, g["ln1"], s("ln1"), z("ln1"), 1, pc)
        sq, zq = s("qkv"), z("qkv")
        w["attn"] = mha_ref.pixels(mha_ref.attention_u8(mha_ref.tokens(g["qkv"]), None, None, 2, sq, zq, sq, zq, sq, zq, f32(score_qp[0]), score_qp[1],
                                                        s("attn"), z("attn"))[3], 1, 5)
        w["proj"] = _dense_ref(proj, g["attn"], s("attn"), z("attn"), 1, pc)
        w["add1"] = add_ref.add_u8(g["pos"], z("pos"), s("pos"), g["proj"], z("proj"), s("proj"), s("add1"), z("add1"))
        w["ln2"] = ln_ref("ln2", g["add1"], "add1")
        w["fc1"] = _dense_ref(fc1, g["ln2"], s("ln2"), z("ln2"), 1, pc)
        w["act"] = act_ref.act_u8(g["fc1"], "hardswish", 0.0, s("fc1"), z("fc1"), s("act"), z("act"))
        w["fc2"] = _dense_ref(fc2, g["act"], s("act"), z("act"), 1, pc)
        w["add2"] = add_ref.add_u8(g["add1"], z("add1"), s("add1"), g["fc2"], z("fc2"), s("fc2"), s("add2"), z("add2"))
        w["ln3"] = ln_ref("ln3", g["add2"], "add2")
        w["cls"] = np.ascontiguousarray(g["ln3"][:, :, :1, :1])
        w["out"] = _dense_ref(head, g["cls"], s("ln3"), z("ln3"), 1, pc).reshape(batch, 5)
        return w

    for fallback in (False, True):
        cx.force_fallback(fallback)
        try:
            out = chain()["out"].numpy()  # nothing but the result observed: every op launches as its consumer asks
            t = chain()
            got = {k: t[k].numpy() for k in reversed(list(t))}
        finally:
            cx.force_fallback(False)
        assert got["pos"].shape == (batch, 16, 1, 5) and got["attn"].shape == (batch, 16, 1, 5) and got["cls"].shape == (batch, 16, 1, 1)
        want = expected(got)
        for k in want:
            assert got[k].shape == want[k].shape and _first_diff(got[k], want[k]) is None, (k, fallback, _first_diff(got[k], want[k]))
        for k in ("pos", "attn", "act", "ln3"):
            assert len(np.unique(got[k])) > 8, (k, np.unique(got[k]))  # (no step has collapsed to a constant)
        assert np.array_equal(out, got["out"]), ("unobserved", fallback)
