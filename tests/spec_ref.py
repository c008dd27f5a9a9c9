"""The numpy interpreter of a `workloads` spec over the oracle: the expected bytes of every network test (DESIGN.md section
2).  A helper module, not a conftest.

Nothing is defined arithmetically here.  Every op is the function of its own module -- the reference's ops in oracle/orc.py,
per-channel requantisation in pc_pipeline, and grouped_ref, add_ref, avgpool_ref, concat_ref, act_ref, mul_ref, deconv_ref,
upsample_ref, dilated_ref, attention_ref, layernorm_ref, mha_ref, groupnorm_ref, padpool_ref for what the reference does not
have -- and
this module only walks the spec with (bytes, scale, zero_point) in hand.  A new op adds one branch to forward(), one to
fp32_qparams() if it is calibrated, its name to OPS, and its arithmetic in a module of its own.

  OPS                                the op names a spec may hold; anything else raises ValueError
  forward(...)                       float32 logits of a network
  fp32_qparams(...)                  stand-in for calibration without a GPU: a float64 forward over the FP32 weights
  quantize_layers(...)               convert()'s weight rules
  outputs_of(name, into)             a trace callback that keeps the output bytes of the ops called `name`
  keeps(keys, into)                  a trace callback that keeps the output bytes of the ops with the given attributes / names
  traces(*callbacks)                 several trace callbacks as one"""
import numpy as np

import act_ref as acr
import add_ref as ar
import attention_ref as atr
import avgpool_ref as apr
import concat_ref as cr
import deconv_ref as dr
import dilated_ref as dl
import f64_ref
import grouped_ref as gr
import groupnorm_ref as gnr
import layernorm_ref as lnr
import mha_ref as mhr
import mul_ref as mr
import orc
import padpool_ref as ppr
import pc_pipeline as pcp
import pipeline
import upsample_ref as ur
from layer_cases import range_qparams  # (the calibrator's rule on a real-valued range)

f32 = np.float32
OPS = frozenset(["layer", "relu", "pool", "avgpool", "gap", "save", "branch", "add", "mul", "concat", "act", "upsample", "flatten",
                 "matmul", "softmax", "load", "attention"])

# synthetic weights, calibration batch and input of the network tests, GPU and host: with them the traced tensors keep the
# limits of act_ref.nontrivial and mul_ref.nontrivial.  (CALIB_IMAGES is the batch of fp32_qparams in the host tests; the GPU
# tests calibrate the product on batches of their own size.)
WEIGHT_SEED, CALIB_SEED, CALIB_IMAGES, INPUT_SEED = 42, 99, 4, 5


def _layer(L, cur, qlayer, s_out, zp_out, per_channel):
    """the output bytes of a weighted layer.  Conv: the reference convolution per group, a dilated kernel inflated by zeros
    (the kernel extent is the weight's); deconv: the reference convolution of the equivalent problem; fc: the reference linear;
    ln, gn: layernorm_ref's LayerNorm and groupnorm_ref's GroupNorm at eps 1e-5, qlayer their float32 (gamma, beta)"""
    q, s, zp = cur
    if L[0] == "ln":
        return lnr.layer_norm_any(q, s, f32(1e-5), qlayer[0], qlayer[1], s_out, zp_out)
    if L[0] == "gn":
        return gnr.group_norm_u8(q, L[1], s, f32(1e-5), qlayer[0], qlayer[1], s_out, zp_out)
    qw, qb, s_w = qlayer
    if L[0] == "conv":
        d = dl.layer_dilation(L)
        f = gr.conv2d_grouped_pc if per_channel else gr.conv2d_grouped
        return f(q, dl.inflate(qw, d) if d > 1 else qw, qb, gr.layer_groups(L), L[4], L[5], s, zp, s_w, s_out, zp_out)[0]
    if L[0] == "deconv":
        f = dr.deconv_u8_pc if per_channel else dr.deconv_u8
        return f(q, qw, qb, L[4], L[5], L[6], s, zp, s_w, s_out, zp_out)[0]
    if L[0] == "fc":
        f = pcp.linear_pc if per_channel else orc.linear
        return f(q.reshape(q.shape[0], -1), qw, qb, s, zp, s_w, s_out, zp_out)[0]
    raise ValueError("spec_ref.forward: layer %r" % (L,))


def forward(networks_entry, x, qlayers, out_qparams, join_qparams=None, per_channel=False, trace=None):
    """x: float32 NCHW.  qlayers: {attr: (qw, qb, s_w)} as quantize_layers gives them (s_w a scalar or, per_channel, float32
    [out]).  out_qparams: {attr: (scale, zp)} of the layers, join_qparams: the same of the Adds, Muls, Concats, Activations,
    MatMuls and Attentions, and under attr + mha_ref.SCORES the score parameters of each Attention.
    trace: called as trace(op, (bytes, scale, zp), operands) behind every op that produces bytes, operands the list of
    (bytes, scale, zp) it read, the current tensor first.  Returns float32 logits."""
    layers, spec, _ = networks_entry

    def run(ops, cur, saved):
        for op in ops:
            (q, s, zp), name = cur, op[0]
            if name == "save":
                saved[op[1]] = cur
                continue
            if name == "branch":
                saved[op[1]] = run(op[2], saved[op[1]], saved)
                continue
            if name == "load":
                cur = saved[op[1]]
                continue
            operands = [cur]
            if name in ("layer", "add", "mul", "concat", "act", "matmul", "attention"):  # the ops with output parameters of their own
                s_out, zp_out = (out_qparams if name == "layer" else join_qparams or {})[op[1]]
                s_out, zp_out = f32(s_out), int(zp_out)
            if name == "layer":
                cur = (_layer(layers[op[1]], cur, qlayers[op[1]], s_out, zp_out, per_channel), s_out, zp_out)
            elif name == "relu":
                cur = (orc.relu(q, zp), s, zp)
            elif name == "pool":  # (a tail -- pad, ceil_mode -- takes padpool_ref's definition; without one, the reference's)
                cur = (ppr.max_pool2d_u8(q, *op[1:]) if len(op) > 3 else orc.max_pool2d(q, op[1], op[2]), s, zp)
            elif name == "avgpool":  # (a padded tap is the byte zp)
                cur = (ppr.avg_pool2d_u8(q, *op[1:], zp=zp) if len(op) > 3 else apr.avg_pool2d_u8(q, op[1], op[1], op[2]), s, zp)
            elif name == "gap":
                cur = (apr.global_avg_pool2d_u8(q), s, zp)
            elif name == "upsample":
                cur = (ur.upsample_u8(q, *ur.factors(op[1]), op[2]), s, zp)
            elif name in ("add", "mul"):
                q2, s2, zp2 = saved[op[2]]
                operands.append(saved[op[2]])
                cur = ((ar.add_u8 if name == "add" else mr.mul_u8)(q, zp, s, q2, zp2, s2, s_out, zp_out, relu=False), s_out, zp_out)
            elif name == "matmul":
                q2, s2, zp2 = saved[op[2]]
                operands.append(saved[op[2]])
                out = atr.matmul_u8(q, zp, s, q2, zp2, s2, s_out, zp_out, transpose_a=op[3], transpose_b=op[4])
                cur = (out.reshape(atr.result_shape(q.shape, q2.shape, op[3], op[4])), s_out, zp_out)
            elif name == "softmax":
                cur = (atr.softmax_u8(q, s), f32(1.0 / 256), 0)
            elif name == "attention":  # [cur], packed, or [q, k, v]
                operands += [saved[t] for t in op[3:]]
                out = mhr.attend_u8(operands, op[2], join_qparams[op[1] + mhr.SCORES], s_out, zp_out)[3]
                cur = (mhr.pixels(out, q.shape[2], q.shape[3]), s_out, zp_out)
            elif name == "concat":
                operands += [saved[t] for t in op[2]]
                cur = (cr.cat_u8(operands, s_out, zp_out), s_out, zp_out)
            elif name == "act":
                kind, param = acr.act_of(op)
                cur = (acr.act_u8(q, kind, param, s, zp, s_out, zp_out), s_out, zp_out)
            elif name == "flatten":
                cur = (q.reshape(-1, op[1]), s, zp)
            else:
                raise ValueError("spec_ref.forward: op %r" % (op,))
            if trace is not None:
                trace(op, cur, operands)
        return cur

    q0 = orc.quantize(x, pipeline.INPUT_SCALE, pipeline.INPUT_ZP)
    return orc.dequantize(*run(spec, (q0, pipeline.INPUT_SCALE, pipeline.INPUT_ZP), {}))


def outputs_of(name, into):
    """a trace callback for forward(): into[attr] = the output bytes of every ("add" | "mul" | "concat" | "act", attr, ...)
    op called `name`.  (mul_ref.tracer, deconv_ref.tracer and upsample_ref.tracer keep what their tests look at.)"""
    def trace(op, out, operands):
        if op[0] == name:
            into[op[1]] = out[0]

    return trace


def keeps(keys, into):
    """a trace callback for forward(): into[key] = the output bytes of every op whose key is in `keys`, the key of an op being
    its attribute name where it has one (layer, add, mul, concat, act, matmul, attention) and its own name otherwise (pool, gap)"""
    def trace(op, out, operands):
        key = op[1] if len(op) > 1 and isinstance(op[1], str) else op[0]
        if key in keys:
            into[key] = out[0]

    return trace


def traces(*callbacks):
    """one trace callback that calls every one of `callbacks`"""
    def trace(op, out, operands):
        for t in callbacks:
            t(op, out, operands)

    return trace


def fp32_qparams(networks_entry, state_dict, x):
    """Stand-in for calibration without a GPU: a numpy forward in float64 over the FP32 weights; the output range of every
    layer, Add, Mul, Concat, Activation, MatMul and Attention gives its (scale, zero_point) by the calibrator's rule, and so does
    the score range of an Attention, kept beside the joins under attr + mha_ref.SCORES.  Pools and upsamples are the float64
    functions of f64_ref, avgpool_ref, padpool_ref and upsample_ref.  Returns (layer qparams, join qparams)."""
    layers, spec, _ = networks_entry
    qp, jqp = {}, {}

    def run(ops, v, saved):
        for op in ops:
            name = op[0]
            if name == "layer":
                L = layers[op[1]]
                w, b = state_dict[op[1] + ".weight"].astype(np.float64), state_dict[op[1] + ".bias"].astype(np.float64)
                if L[0] == "ln":  # over the channel axis: axis 1 of [n, c, h, w], the last of [n, f]
                    rows = np.ascontiguousarray(np.moveaxis(v, 1, -1))
                    v = np.ascontiguousarray(np.moveaxis(lnr.layer_norm_f64(rows, w, b, 1e-5), -1, 1))
                elif L[0] == "gn":
                    v = gnr.group_norm_f64(v, L[1], w, b, 1e-5)
                elif L[0] == "conv":
                    v = gr.conv2d_f64(v, dl.inflate(w, dl.layer_dilation(L)), b, gr.layer_groups(L), L[4], L[5])
                elif L[0] == "deconv":
                    v = dr.scatter(v, w, b, L[4], L[5], L[6])
                else:
                    v = f64_ref.linear(v.reshape(v.shape[0], -1), w, b)
            elif name == "act":
                kind, param = acr.act_of(op)
                v = acr.act_f64(kind, v, param)
            elif name == "relu":
                v = np.maximum(v, 0.0)
            elif name == "pool":
                v = ppr.max_pool2d_f64(v, *op[1:]) if len(op) > 3 else f64_ref.max_pool2d(v, op[1], op[2])
            elif name == "avgpool":
                v = (ppr.avg_pool2d_f64(v, *op[1:]) if len(op) > 3 else apr.avg_pool2d_f64(v, op[1], op[1], op[2]))[0]
            elif name == "upsample":
                fh, fw = ur.factors(op[1])
                v = ur.bilinear_f64(v, fh, fw)[0] if op[2] == "bilinear" else ur.nearest(v, fh, fw)
            elif name == "save":
                saved[op[1]] = v
            elif name == "branch":
                saved[op[1]] = run(op[2], saved[op[1]], saved)
            elif name == "add":
                v = v + saved[op[2]]
            elif name == "mul":
                v = v * mr.as_gate(v, saved[op[2]])
            elif name == "load":
                v = saved[op[1]]
            elif name == "matmul":
                v2 = saved[op[2]]
                v = atr.matmul(v, v2, op[3], op[4])[0].reshape(atr.result_shape(v.shape, v2.shape, op[3], op[4]))
            elif name == "softmax":
                v = atr.softmax(v)
            elif name == "attention":
                toks = [mhr.tokens(a) for a in [v] + [saved[tag] for tag in op[3:]]]
                scores, out = mhr.attention(toks[0], *(toks[1:] or (None, None)), op[2])
                jqp[op[1] + mhr.SCORES] = range_qparams(scores.min(), scores.max())
                v = mhr.pixels(out, v.shape[2], v.shape[3])
            elif name == "concat":
                v = np.concatenate([v] + [saved[t] for t in op[2]], axis=1)
            elif name == "gap":
                v = v.mean(axis=(2, 3), keepdims=True)
            elif name == "flatten":
                v = v.reshape(-1, op[1])
            else:
                raise ValueError("spec_ref.fp32_qparams: op %r" % (op,))
            if name in ("layer", "act", "add", "mul", "concat", "matmul", "attention"):
                (qp if name == "layer" else jqp)[op[1]] = range_qparams(v.min(), v.max())
        return v

    run(spec, np.asarray(x, np.float64), {})
    return qp, jqp


def quantize_layers(networks_entry, state_dict, per_channel=False):
    """{attr: (qw, qb, s_w)} by convert()'s rules on the weight tensors as they stand ([kc, c / groups, kh, kw] of a grouped
    conv, the compact kernel of a dilated one), a "deconv" layer as its equivalent kernel W~ [out, in, k, k]: per tensor the
    oracle's joint min / max over the whole weight and the bias, per channel the same per row of the [kc, K] matrix.  An "ln"
    or "gn" layer has no INT8 weights: its float32 (weight, bias) as they stand."""
    rule = pcp.quantize_weight_pc if per_channel else orc.quantize_weight
    out = {}
    for attr, L in networks_entry[0].items():
        w, b = state_dict[attr + ".weight"], state_dict[attr + ".bias"]
        out[attr] = (w, b) if L[0] in ("ln", "gn") else tuple(rule(dr.equivalent_weight(w) if L[0] == "deconv" else w, b))
    return out
