"""What every bit-exact network test on the GPU shares (tests/test_gpu_add.py ... test_gpu_dilated.py): the calibrated network
with what tests/spec_ref.py needs to restate it, and the comparison of the product's output with the expected bytes -- eager,
under the force-fallback option, replayed as a HIP graph, and after a save / load round trip.  A test keeps what is its own:
its input, its traced tensors and their limits, its shapes and counts."""
import spec_ref as sr
from support import same_bits

_CALIBRATED = {}


def qparams_of(net, key):
    """output_qparams() of the module `key` names, or the score_qparams() of the Attention a key attr + mha_ref.SCORES names"""
    scores = key.endswith(sr.mhr.SCORES)
    return getattr(net, key[:-len(sr.mhr.SCORES)]).score_qparams() if scores else getattr(net, key).output_qparams()


def calibrated(name, per_channel, calib_images=None, mode=None):
    """(net, qlayers, qp, jqp) of network `name` with the synthetic weights of sr.WEIGHT_SEED, calibrated once per argument
    tuple.  calib_images: None for workloads.calibrated's own batch, or the number of images of sr.CALIB_SEED.  mode: a
    calibration mode ("host", "device") for this calibration alone; "auto" and an unseeded calibrator are put back behind it.
    qp holds the output_qparams() of wl.layer_names(name), jqp those of wl.join_names(name) and, as spec_ref.forward reads
    them, the score_qparams() of wl.attention_names(name)."""
    import _CXX_i8ie as cx
    from int8inferenceengine_amd import workloads as wl

    key = (name, per_channel, calib_images, mode)
    if key not in _CALIBRATED:
        sd = wl.synthetic_state_dict(name, sr.WEIGHT_SEED)
        batch = None if calib_images is None else wl.synthetic_input(name, calib_images, seed=sr.CALIB_SEED)
        if mode is not None:
            cx.set_calibration_mode(mode)
        try:
            net = wl.calibrated(name, sd, calib_batch=batch, per_channel=per_channel)  # (under calibration seed 7)
        finally:
            if mode is not None:
                cx.set_calibration_mode("auto")
                cx.set_calibration_seed(-1)
        qp = {a: getattr(net, a).output_qparams() for a in wl.layer_names(name)}
        jqp = {a: qparams_of(net, a) for a in wl.join_names(name) + [a + sr.mhr.SCORES for a in wl.attention_names(name)]}
        _CALIBRATED[key] = (net, sr.quantize_layers(wl.network(name), sd, per_channel), qp, jqp)
    return _CALIBRATED[key]


def check_bit_exact(i8ie, net, name, x, want, *, fallback=False, graph=False, reload_dir=None, expect_jqp=None):
    """net(x) is `want` bit for bit; returns the eager output.  fallback: also under cx.force_fallback(True).  graph: also two
    replays of the forward captured as one HIP graph.  reload_dir: also a fresh wl.build(name) that loaded what
    net.save_quantized() wrote there, which then answers expect_jqp (name -> output_qparams(), attr + mha_ref.SCORES ->
    score_qparams()) as well."""
    import _CXX_i8ie as cx
    from int8inferenceengine_amd import workloads as wl
    from int8inferenceengine_amd.graph import GraphedForward

    got = net(i8ie.tensor(x)).numpy()
    assert same_bits(got, want), "eager"
    if fallback:
        cx.force_fallback(True)
        try:
            fb = net(i8ie.tensor(x)).numpy()
        finally:
            cx.force_fallback(False)
        assert same_bits(fb, want), "force_fallback"
    if graph:
        g = GraphedForward(net, i8ie.tensor(x).prefetch())
        for _ in range(2):
            assert same_bits(g().numpy(), want), "graph replay"
    if reload_dir is not None:
        path = str(reload_dir / (name + ".npz"))
        net.save_quantized(path)
        fresh = wl.build(name)
        fresh.load_quantized_file(path)
        assert {a: qparams_of(fresh, a) for a in expect_jqp or {}} == (expect_jqp or {})
        assert same_bits(fresh(i8ie.tensor(x)).numpy(), want), "reloaded"
    return got


def traced(i8ie, net, name, x, trace):
    """The product's own tensors where spec_ref.forward traces its main path: the top-level spec of network `name` walked op by
    op through net.run, and `trace` -- a spec_ref trace callback that looks at the op and the output bytes only -- called
    behind every op that produces a tensor, as trace(op, (bytes, scale, zero_point), None)."""
    from int8inferenceengine_amd import workloads as wl

    cur, saved = i8ie.quantize(i8ie.tensor(x), float(sr.pipeline.INPUT_SCALE), sr.pipeline.INPUT_ZP), {}
    for op in wl.network(name)[1]:
        cur = net.run([op], cur, saved)
        if op[0] not in ("save", "branch", "load"):
            trace(op, (cur.numpy(), cur.scale, cur.zero_point), None)
