// operands.h -- the operand rules of the deferred quantized ops, pinned by tests/test_gpu_operand_rules.py.
#pragma once
#include "tensor.h"

namespace i8ie_py {

void check_zero_point(int zp);
// the result's quantisation parameters as a caller of add / mul / cat / lut gave them
void check_out_qparams(const char* op, float scale, int zp);
// an op that refuses a default-constructed tensor does so before anything is recorded
inline void need_contents(const Tensor<u8_t>& t) {
  if (!t.st && !t.pend) throw std::runtime_error("i8ie: empty tensor");
}
// ---- the operand rules of the deferred joining ops (add, mul, cat, lut, avg_pool2d) ----------------
// The storage an operand is read from, as it lies (any layout, border, re-bias).  A producer that has launched for another
// consumer -- the skip tensor, made bordered / re-biased for the first conv of the block -- is taken from its node's results;
// one that has not launches plain.
std::shared_ptr<Storage> operand_as_it_lies(Tensor<u8_t>& t);
// `t` must not launch before `reader`: both are pending and reader = f(t) has not launched.  Launching the reader launches t
// for f (bordered as f wants it), and t is then found among its node's results instead of launching a second time, plain.
bool waits_for(const Tensor<u8_t>& t, const Tensor<u8_t>& reader);
// The storages of k operands, as they lie: each round launches the first unresolved operand that waits for no other unresolved
// one.  Two operands: b goes first exactly when waits_for(a, b) -- a then finds waits_for(b, a) false, which a cycle alone could
// make true, and a cycle cannot be recorded -- and a goes first otherwise.
std::vector<std::shared_ptr<Storage>> resolve_operands(Tensor<u8_t>* ts, size_t k);
// NCHW operands converted for one launch: (source, its NHWC copy).  Lives as long as the launch is being queued.
using NhwcCopies = std::vector<std::pair<std::shared_ptr<Storage>, std::shared_ptr<Storage>>>;
// A rank-4 operand in the engine's layout under the logical dims `shp`.  A view whose storage is NHWC under other logical dims
// goes back to the reference's order first (the view is defined on it); an NCHW tensor (user-made) takes one conversion into a
// temporary that `copies` keeps alive, and the same storage coming again gets the same copy.
std::shared_ptr<Storage> as_engine_nhwc(const std::shared_ptr<Storage>& s, const std::vector<ssize_t>& shp, NhwcCopies& copies);
// Two operands of one shape brought to one layout (add, the equal-shape mul).  Operands that agree stay as they lie: two NCHW
// tensors take the flat form.  Rank 4 otherwise: the engine keeps NHWC between layers (and a consumer that asked for a border
// reads NHWC).  Other ranks -- a flattened NHWC activation against plain rows -- both back to the reference's order.
void reconcile_pair(std::shared_ptr<Storage>& sa, std::shared_ptr<Storage>& sb, const std::vector<ssize_t>& shp, NhwcCopies& copies);

// The deferred result of an op on one u8 tensor (avg_pool2d, upsample, lut, layer_norm).  relu(op(..)) is one launch, a consuming
// conv gets its zero-point border and, where it reads them, re-biased bytes straight from the op's kernel, and several consumers
// share one launch (PendNode).  body(si, relu, border, s8) launches on the operand as it lies and returns the result's storage.
template <typename Body>
Tensor<u8_t> deferred_one_input(Tensor<u8_t>& in, std::vector<ssize_t> shape, float scale, u8_t zp, Body body) {
  Tensor<u8_t> out = pending_u8(std::move(shape), scale, zp);
  Tensor<u8_t> src = in;  // shares the input's storage / pending launch
  out.pend = make_pend([src, body](bool relu, int border, bool s8) mutable { return body(operand_as_it_lies(src), relu, border, s8); },
                       {in.pend});
  return out;
}

}  // namespace i8ie_py
