// PyTorch bindings of the gfx950 kernels + RCCL reducer.  Every entry point validates device/dtype/contiguity/shape
// before launching — a hand-written kernel must never see an operand whose shape its grid does not assume.
//
// The only translation unit that includes torch headers, and deliberately ONE: parsing those headers costs about
// three times as long as compiling everything below them (and longer than the slowest kernel file), so a per-subject
// split would pay that parse once per file for a few seconds of own code each.
//
// Layout: the operand vocabulary (Op), then one section per heading of hq_kernels.h with each --precision fp32 twin
// next to its bf16 op, then the module definition.  A binding names its dimensions once, gives every tensor its
// launcher dereferences one Op line in those names, then allocates and launches.
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include <array>
#include <limits>
#include <map>

#include "hq_kernels.h"
#include "hq_reducer.h"

namespace {

using at::Tensor;
using OptTensor = c10::optional<Tensor>;

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

bool has(const OptTensor& t) { return t.has_value() && t->defined(); }
template <typename T>
T* ptr(const Tensor& t) { return reinterpret_cast<T*>(t.data_ptr()); }
template <typename T>
T* optr(const OptTensor& t) { return has(t) ? reinterpret_cast<T*>(t->data_ptr()) : nullptr; }

const auto BF16 = at::kBFloat16;
const auto F32 = at::kFloat;
const auto I64 = at::kLong;
const auto I32 = at::kInt;
const auto E4M3 = at::kFloat8_e4m3fn;
const auto E5M2 = at::kFloat8_e5m2;
constexpr int64_t kU32Max = std::numeric_limits<uint32_t>::max();

// ---------------------------------------------------------------------------------- operand contract
// One binding's operand checks, built from the op's name and its first tensor.  Every operand line verifies ALL of:
// on the first operand's (GPU) device, the exact dtype, contiguous, and the exact sizes (`is`) or — where the kernel
// only needs a count — the element count (`holds`).  An optional operand gets the same checks when it is present.
// Failures read "<op>: <operand> <what it is>, expected <what>".
struct Op {
  const char* op;
  c10::Device dev;
  Op(const char* op_, const Tensor& first) : op(op_), dev(first.device()) {
    TORCH_CHECK(dev.is_cuda(), op, ": the first tensor operand is on ", dev, ", expected a GPU tensor");
  }
  // the [rows, cols] a matrix operand brings to the op's dimension names; its own `is` line then pins the rest
  std::array<int64_t, 2> matrix(const Tensor& t, const char* name) const {
    TORCH_CHECK(t.dim() == 2, op, ": ", name, " has ", t.dim(), " dimensions, expected 2");
    return {t.size(0), t.size(1)};
  }
  // device and dtype alone: the part the strided bindings (gemm_f32, qa_decode) take from here
  void on(const Tensor& t, at::ScalarType dt, const char* name) const {
    TORCH_CHECK(t.device() == dev, op, ": ", name, " is on ", t.device(), ", expected ", dev);
    TORCH_CHECK(t.scalar_type() == dt, op, ": ", name, " has dtype ", t.scalar_type(), ", expected ", dt);
  }
  // + contiguous: an operand whose own element count is the dimension (or whose contents carry their extents)
  void dense(const Tensor& t, at::ScalarType dt, const char* name) const {
    on(t, dt, name);
    TORCH_CHECK(t.is_contiguous(), op, ": ", name, " has strides ", t.strides(), " for sizes ", t.sizes(),
                ", expected contiguous");
  }
  void is(const Tensor& t, at::ScalarType dt, const char* name, at::IntArrayRef sizes) const {
    dense(t, dt, name);
    TORCH_CHECK(t.sizes() == sizes, op, ": ", name, " has sizes ", t.sizes(), ", expected ", sizes);
  }
  void holds(const Tensor& t, at::ScalarType dt, const char* name, int64_t n) const {
    dense(t, dt, name);
    TORCH_CHECK(t.numel() == n, op, ": ", name, " has ", t.numel(), " elements, expected ", n);
  }
  // a scalar the kernel reads at [0] out of a possibly longer vector (fp8 scales, the dropout seed)
  void at_least(const Tensor& t, at::ScalarType dt, const char* name, int64_t n) const {
    dense(t, dt, name);
    TORCH_CHECK(t.numel() >= n, op, ": ", name, " has ", t.numel(), " elements, expected at least ", n);
  }
  void is(const OptTensor& t, at::ScalarType dt, const char* name, at::IntArrayRef sizes) const {
    if (has(t)) is(*t, dt, name, sizes);
  }
  void holds(const OptTensor& t, at::ScalarType dt, const char* name, int64_t n) const {
    if (has(t)) holds(*t, dt, name, n);
  }
  // an fp8 site's f32[4] delayed-scaling state -> the kernels' pointer (null when absent)
  float* state4(const OptTensor& t, const char* name) const {
    if (!has(t)) return nullptr;
    holds(*t, F32, name, 4);
    return ptr<float>(*t);
  }
};

// a buffer of 1-byte elements (uint8 and float8 views of the same bytes): its own dtype if that is one byte wide
at::ScalarType byte_dtype(const Tensor& t) { return t.element_size() == 1 ? t.scalar_type() : at::kByte; }

// Row-wise ops over [T, H] (embedding, LayerNorm, forward and backward alike).  Hidden sizes the kernels take —
// bf16: four columns per lane step, up to 2048; fp32: any width up to 1024 (dispatch_nc) — and the 32-bit element
// index of the dropout stream.
void check_rows(const Op& c, at::ScalarType dt, int64_t T, int64_t H) {
  if (dt == BF16) {
    TORCH_CHECK(H >= 4 && H % 4 == 0 && H <= 2048, c.op, ": hidden size is ", H, ", expected a multiple of 4 and <= 2048");
  } else {
    TORCH_CHECK(H >= 1 && H <= 1024, c.op, ": hidden size is ", H, ", expected 1..1024 for the fp32 row kernels");
  }
  TORCH_CHECK(T * H < kU32Max, c.op, ": T*H is ", T * H, ", expected to fit the 32-bit dropout index");
}

HqOuts outs4(float* a, float* b = nullptr, float* c = nullptr, float* d = nullptr) { return HqOuts{{a, b, c, d}}; }

uint32_t u32(int64_t v) { return (uint32_t)(v & 0xFFFFFFFFll); }

// ------------------------------------------- rowops.hip: process-wide state, element-wise ops, column sums
void set_dropout_seed(OptTensor t) {
  if (!has(t)) { hq_set_dropout_seed_ptr(nullptr); return; }
  const Op c("set_dropout_seed", *t);
  c.at_least(*t, I32, "seed", 1);
  hq_set_dropout_seed_ptr(reinterpret_cast<const uint32_t*>(t->data_ptr()));
}

// bool / uint8 attention mask -> fp32 additive key bias, same shape
Tensor key_bias(Tensor mask) {
  const Op c("key_bias", mask);
  c.dense(mask, mask.scalar_type() == at::kByte ? at::kByte : at::kBool, "mask");
  c10::DeviceGuard g(c.dev);
  auto kb = at::empty(mask.sizes(), mask.options().dtype(F32));
  hq_key_bias(reinterpret_cast<const uint8_t*>(mask.data_ptr()), ptr<float>(kb), (int)mask.numel(), cur_stream());
  return kb;
}

Tensor gelu_fwd(Tensor pre) {
  const Op c("gelu_fwd", pre);
  c.dense(pre, BF16, "pre");
  TORCH_CHECK(pre.numel() % 8 == 0, "gelu_fwd: pre has ", pre.numel(), " elements, expected a multiple of 8");
  c10::DeviceGuard g(c.dev);
  auto out = at::empty_like(pre);
  hq_gelu_fwd(ptr<uint16_t>(pre), ptr<uint16_t>(out), pre.numel(), cur_stream());
  return out;
}

Tensor f32_gelu_fwd(Tensor x) {
  const Op c("f32_gelu_fwd", x);
  c.dense(x, F32, "x");
  c10::DeviceGuard g(c.dev);
  auto y = at::empty_like(x);
  hq_f32_gelu_fwd(ptr<float>(x), ptr<float>(y), x.numel(), cur_stream());
  return y;
}

// gelu_bwd / f32_gelu_bwd: dout, pre [T, N] of `dt`; g_bias f32 [N] optional
struct RowDims { int64_t T, N; };
RowDims gelu_bwd_operands(const Op& c, at::ScalarType dt, const Tensor& dout, const Tensor& pre, const OptTensor& g_bias) {
  const auto [T, N] = c.matrix(dout, "dout");
  c.is(dout, dt, "dout", {T, N});
  c.is(pre, dt, "pre", {T, N});
  c.holds(g_bias, F32, "g_bias", N);
  if (dt == BF16) TORCH_CHECK(N % 8 == 0, c.op, ": N is ", N, ", expected a multiple of 8");
  return {T, N};
}

Tensor gelu_bwd(Tensor dout, Tensor pre, OptTensor g_bias, bool accumulate) {
  const Op c("gelu_bwd", dout);
  const auto [T, N] = gelu_bwd_operands(c, BF16, dout, pre, g_bias);
  c10::DeviceGuard g(c.dev);
  auto dpre = at::empty_like(dout);
  auto part = at::empty({hq_rowblock_partials((int)T), N}, dout.options().dtype(F32));
  hq_gelu_bwd(ptr<uint16_t>(dout), ptr<uint16_t>(pre), ptr<uint16_t>(dpre), ptr<float>(part), outs4(optr<float>(g_bias)),
              (int)T, (int)N, accumulate, cur_stream());
  return dpre;
}

Tensor f32_gelu_bwd(Tensor dout, Tensor x, OptTensor g_bias, bool accumulate) {
  const Op c("f32_gelu_bwd", dout);
  const auto [T, N] = gelu_bwd_operands(c, F32, dout, x, g_bias);
  c10::DeviceGuard g(c.dev);
  auto d = at::empty_like(x);
  auto part = at::empty({hq_f32_part_rows((int)T), N}, x.options());
  hq_f32_gelu_bwd(ptr<float>(dout), ptr<float>(x), ptr<float>(d), ptr<float>(part), optr<float>(g_bias), (int)T, (int)N,
                  accumulate, cur_stream());
  return d;
}

void bias_grad(Tensor dy, Tensor g_b, bool accumulate) {
  const Op c("bias_grad", dy);
  const auto [T, N] = c.matrix(dy, "dy");
  c.is(dy, BF16, "dy", {T, N});
  c.holds(g_b, F32, "g_b", N);
  TORCH_CHECK(N % 8 == 0, "bias_grad: N is ", N, ", expected a multiple of 8");
  c10::DeviceGuard g(c.dev);
  auto part = at::empty({hq_rowblock_partials((int)T), N}, g_b.options());
  hq_bias_grad(ptr<uint16_t>(dy), ptr<float>(part), outs4(ptr<float>(g_b)), (int)T, (int)N, accumulate, cur_stream());
}

void f32_colsum(Tensor x, Tensor out, bool accumulate) {
  const Op c("f32_colsum", x);
  const auto [T, N] = c.matrix(x, "x");
  c.is(x, F32, "x", {T, N});
  c.holds(out, F32, "out", N);
  c10::DeviceGuard g(c.dev);
  auto part = at::empty({hq_f32_part_rows((int)T), N}, x.options());
  hq_f32_colsum(ptr<float>(x), ptr<float>(part), ptr<float>(out), (int)T, (int)N, accumulate, cur_stream());
}

// out (+)= Σ_rows part.  `part` is scratch: the two-pass reduction overwrites some of its rows.
void colsum_into(Tensor part, Tensor out, bool accumulate) {
  const Op c("colsum_into", part);
  const auto [P, N] = c.matrix(part, "part");
  c.is(part, F32, "part", {P, N});
  c.holds(out, F32, "out", N);
  c10::DeviceGuard g(c.dev);
  hq_colsum(ptr<float>(part), (int)P, (int)N, ptr<float>(out), accumulate, cur_stream());
}

// ------------------------------------------------- norm.hip, f32_norm.hip: residual + dropout + LayerNorm
// ln_fwd / f32_ln_fwd: a [T, H] of `dt`, resid the same (bf16: optional), gamma / beta f32 [H]
struct LnDims { int64_t T, H; };
LnDims ln_fwd_operands(const Op& c, at::ScalarType dt, const Tensor& a, const OptTensor& resid, const Tensor& gamma,
                       const Tensor& beta) {
  const auto [T, H] = c.matrix(a, "a");
  c.is(a, dt, "a", {T, H});
  c.is(resid, dt, "resid", {T, H});
  c.holds(gamma, F32, "gamma", H);
  c.holds(beta, F32, "beta", H);
  check_rows(c, dt, T, H);
  return {T, H};
}

// ln_bwd / f32_ln_bwd: dy, z (and dy2) [T, H] of `dt`; gamma (and beta) f32 [H]; mean / rstd f32 [T]; the
// optional gradient vectors f32 [H]
LnDims ln_bwd_operands(const Op& c, at::ScalarType dt, const Tensor& dy, const OptTensor& dy2, const Tensor& z,
                       const Tensor& gamma, const Tensor& mean, const Tensor& rstd, const OptTensor& g_gamma,
                       const OptTensor& g_beta, const OptTensor& g_bias, const OptTensor& beta) {
  const auto [T, H] = c.matrix(dy, "dy");
  c.is(dy, dt, "dy", {T, H});
  c.is(dy2, dt, "dy2", {T, H});
  c.is(z, dt, "z", {T, H});
  c.holds(gamma, F32, "gamma", H);
  c.holds(beta, F32, "beta", H);
  c.holds(mean, F32, "mean", T);
  c.holds(rstd, F32, "rstd", T);
  c.holds(g_gamma, F32, "g_gamma", H);
  c.holds(g_beta, F32, "g_beta", H);
  c.holds(g_bias, F32, "g_bias", H);
  check_rows(c, dt, T, H);
  return {T, H};
}

// With q8 (f32[4] delayed-scaling state of the consuming fp8 GEMM's input): also returns y as e4m3.
// resid = None: `a` already is z (EPI_BDR GEMM epilogue) -> returns {y, a, mean, rstd} without touching z
// store_z = false: z is not written (returned empty) — the backward then recomputes x̂ from y (ln_bwd beta=)
std::vector<Tensor> ln_fwd(Tensor a, OptTensor resid_opt, Tensor gamma, Tensor beta, double eps, double p, int64_t seed,
                           int64_t opid, OptTensor q8, int64_t phase, bool store_z) {
  const Op c("ln_fwd", a);
  const auto [T, H] = ln_fwd_operands(c, BF16, a, resid_opt, gamma, beta);
  const bool zin = !has(resid_opt), want8 = has(q8);
  TORCH_CHECK(!(zin && want8), "ln_fwd: the z-in form has no e4m3 output");
  float* q8p = c.state4(q8, "q8");
  c10::DeviceGuard g(c.dev);
  auto y = at::empty_like(a);
  const bool wz = zin || store_z;
  auto z = zin ? a : (store_z ? at::empty_like(a) : at::empty({0}, a.options()));
  auto mean = at::empty({T}, gamma.options()), rstd = at::empty({T}, gamma.options());
  Tensor y8 = want8 ? at::empty({T, H}, a.options().dtype(E4M3)) : Tensor();
  hq_ln_fwd(ptr<uint16_t>(a), zin ? nullptr : ptr<uint16_t>(*resid_opt), ptr<float>(gamma), ptr<float>(beta),
            ptr<uint16_t>(y), (zin || !wz) ? nullptr : ptr<uint16_t>(z),
            ptr<float>(mean), ptr<float>(rstd), (int)T, (int)H, (float)eps, (float)p, u32(seed), u32(opid), cur_stream(),
            want8 ? reinterpret_cast<uint8_t*>(y8.data_ptr()) : nullptr, q8p, (int)(phase % 3));
  if (want8) return {y, z, mean, rstd, y8};
  return {y, z, mean, rstd};
}

std::vector<Tensor> f32_ln_fwd(Tensor a, Tensor resid, Tensor gamma, Tensor beta, double eps, double p, int64_t seed,
                               int64_t opid) {
  const Op c("f32_ln_fwd", a);
  const auto [T, H] = ln_fwd_operands(c, F32, a, resid, gamma, beta);
  c10::DeviceGuard g(c.dev);
  auto y = at::empty_like(a), z = at::empty_like(a);
  auto mean = at::empty({T}, a.options()), rstd = at::empty({T}, a.options());
  hq_f32_ln_fwd(ptr<float>(a), ptr<float>(resid), ptr<float>(gamma), ptr<float>(beta), ptr<float>(y), ptr<float>(z),
                ptr<float>(mean), ptr<float>(rstd), (int)T, (int)H, (float)eps, (float)p, u32(seed), u32(opid), cur_stream());
  return {y, z, mean, rstd};
}

// beta given: `z` is the forward OUTPUT y and x̂ = (y − β)/γ (the forward ran with store_z = false)
// q8 (f32[4] delayed-scaling state of the fp8 dgrad GEMM that consumes da): also returns da as e5m2;
// write_da = false (with q8): da only as e5m2 — the bf16 da comes back empty
std::vector<Tensor> ln_bwd(Tensor dy, OptTensor dy2, Tensor z, Tensor gamma, Tensor mean, Tensor rstd, double p, int64_t seed,
                           int64_t opid, OptTensor g_gamma, OptTensor g_beta, OptTensor g_bias, bool accumulate,
                           OptTensor q8, int64_t phase, bool write_da, OptTensor beta) {
  const Op c("ln_bwd", dy);
  const auto [T, H] = ln_bwd_operands(c, BF16, dy, dy2, z, gamma, mean, rstd, g_gamma, g_beta, g_bias, beta);
  const bool want8 = has(q8);
  TORCH_CHECK(write_da || want8, "ln_bwd: write_da=False needs q8");
  float* q8p = c.state4(q8, "q8");
  c10::DeviceGuard g(c.dev);
  auto dz = at::empty_like(dy), da = write_da ? at::empty_like(dy) : at::empty({0}, dy.options());
  const int nb = hq_ln_bwd_partials((int)T);
  auto part = at::empty({nb, 3 * H}, gamma.options());
  Tensor da8 = want8 ? at::empty(dy.sizes(), dy.options().dtype(E5M2)) : Tensor();
  hq_ln_bwd(ptr<uint16_t>(dy), optr<uint16_t>(dy2), ptr<uint16_t>(z), ptr<float>(gamma), ptr<float>(mean), ptr<float>(rstd),
            ptr<uint16_t>(dz), write_da ? ptr<uint16_t>(da) : nullptr, ptr<float>(part),
            outs4(optr<float>(g_gamma), optr<float>(g_beta), optr<float>(g_bias)), (int)T, (int)H, (float)p, u32(seed),
            u32(opid), accumulate, cur_stream(), want8 ? reinterpret_cast<uint8_t*>(da8.data_ptr()) : nullptr,
            q8p, (int)(phase % 3), optr<float>(beta));
  if (want8) return {dz, da, da8};
  return {dz, da};
}

std::vector<Tensor> f32_ln_bwd(Tensor dy, OptTensor dy2, Tensor z, Tensor gamma, Tensor mean, Tensor rstd, double p,
                               int64_t seed, int64_t opid, OptTensor g_gamma, OptTensor g_beta, OptTensor g_bias,
                               bool accumulate, OptTensor beta) {
  const Op c("f32_ln_bwd", dy);
  const auto [T, H] = ln_bwd_operands(c, F32, dy, dy2, z, gamma, mean, rstd, g_gamma, g_beta, g_bias, beta);
  c10::DeviceGuard g(c.dev);
  auto dz = at::empty_like(dy), da = at::empty_like(dy);
  auto part = at::empty({hq_f32_part_rows((int)T), 3 * H}, dy.options());
  hq_f32_ln_bwd(ptr<float>(dy), optr<float>(dy2), ptr<float>(z), ptr<float>(gamma), optr<float>(beta), ptr<float>(mean),
                ptr<float>(rstd), ptr<float>(dz), ptr<float>(da), ptr<float>(part),
                outs4(optr<float>(g_gamma), optr<float>(g_beta), optr<float>(g_bias)), (int)T, (int)H, (float)p, u32(seed),
                u32(opid), accumulate, cur_stream());
  return {dz, da};
}

// flags[i]: LayerNorm i's γ / β ratio test.  The offsets are validated against the arena on the host when the
// caller builds them: no device read here.
Tensor ln_guard(Tensor master, Tensor goff, Tensor boff, int64_t H, double ratio) {
  const Op c("ln_guard", master);
  const int64_t n = goff.numel();
  c.dense(master, F32, "master");
  c.holds(goff, I64, "goff", n);
  c.holds(boff, I64, "boff", n);
  c10::DeviceGuard g(c.dev);
  auto flags = at::empty({n}, master.options().dtype(at::kBool));
  hq_ln_guard(ptr<float>(master), goff.data_ptr<int64_t>(), boff.data_ptr<int64_t>(), (int)n, (int)H, (float)ratio,
              reinterpret_cast<uint8_t*>(flags.data_ptr()), cur_stream());
  return flags;
}

// ------------------------------------------------------------------------------------- sort.hip
// the embedding backward's stable id sort (tests): (sorted keys, their rows)
std::pair<Tensor, Tensor> sort_ids(Tensor ids, int64_t V) {
  const Op c("sort_ids", ids);
  const int T = (int)ids.numel();
  c.is(ids, I64, "ids", {(int64_t)T});
  c10::DeviceGuard g(c.dev);
  auto buf = at::empty({4, std::max(T, 1)}, ids.options().dtype(I32));
  auto hist = at::empty({(int64_t)std::max<size_t>(hq_sort_ids_bytes(T, (int)V), 4)}, ids.options().dtype(at::kByte));
  int32_t* b = buf.data_ptr<int32_t>();
  const int64_t stride = std::max(T, 1);
  hq_sort_ids(ids.data_ptr<int64_t>(), T, (int)V, b, b + stride, b + 2 * stride, b + 3 * stride, hist.data_ptr(),
              hist.numel(), cur_stream());
  return std::make_pair(buf[2].narrow(0, 0, T), buf[3].narrow(0, 0, T));
}

// ------------------------------------------------------------------------ embed.hip, f32_embed.hip
// What forward and backward of both precisions share: ids / pos_ids / type_ids int64 with T elements; the tables
// w_word [V, H], w_pos [P, H], w_type [NT, H] of `dt`; gamma f32 [H].
struct EmbDims { int64_t T, H, V, P, NT; };
EmbDims embed_operands(const Op& c, at::ScalarType dt, const Tensor& ids, const Tensor& pids, const Tensor& tids,
                       const Tensor& ww, const Tensor& wp, const Tensor& wt, const Tensor& gamma) {
  const auto [V, H] = c.matrix(ww, "w_word");
  const EmbDims d{ids.numel(), H, V, c.matrix(wp, "w_pos")[0], c.matrix(wt, "w_type")[0]};
  c.dense(ids, I64, "ids");
  c.holds(pids, I64, "pos_ids", d.T);
  c.holds(tids, I64, "type_ids", d.T);
  c.is(ww, dt, "w_word", {d.V, d.H});
  c.is(wp, dt, "w_pos", {d.P, d.H});
  c.is(wt, dt, "w_type", {d.NT, d.H});
  c.holds(gamma, F32, "gamma", d.H);
  check_rows(c, dt, d.T, d.H);
  return d;
}

// + the backward's own: dy [T, H] of `dt`, mean / rstd f32 [T], the table gradients f32 in their tables' shapes,
// g_gamma / g_beta f32 [H]
EmbDims embed_bwd_operands(const Op& c, at::ScalarType dt, const Tensor& dy, const Tensor& ids, const Tensor& pids,
                           const Tensor& tids, const Tensor& ww, const Tensor& wp, const Tensor& wt, const Tensor& gamma,
                           const Tensor& mean, const Tensor& rstd, const Tensor& g_word, const Tensor& g_pos,
                           const Tensor& g_type, const Tensor& g_gamma, const Tensor& g_beta) {
  const EmbDims d = embed_operands(c, dt, ids, pids, tids, ww, wp, wt, gamma);
  c.is(dy, dt, "dy", {d.T, d.H});
  c.holds(mean, F32, "mean", d.T);
  c.holds(rstd, F32, "rstd", d.T);
  c.is(g_word, F32, "g_word", {d.V, d.H});
  c.is(g_pos, F32, "g_pos", {d.P, d.H});
  c.is(g_type, F32, "g_type", {d.NT, d.H});
  c.holds(g_gamma, F32, "g_gamma", d.H);
  c.holds(g_beta, F32, "g_beta", d.H);
  return d;
}

std::vector<Tensor> embed_fwd(Tensor ids, Tensor pids, Tensor tids, Tensor ww, Tensor wp, Tensor wt, Tensor gamma,
                              Tensor beta, double eps, double p, int64_t seed, int64_t opid) {
  const Op c("embed_fwd", ids);
  const EmbDims d = embed_operands(c, BF16, ids, pids, tids, ww, wp, wt, gamma);
  c.holds(beta, F32, "beta", d.H);
  c10::DeviceGuard g(c.dev);
  auto y = at::empty({d.T, d.H}, ww.options());
  auto mean = at::empty({d.T}, gamma.options());
  auto rstd = at::empty({d.T}, gamma.options());
  hq_embed_fwd(ptr<int64_t>(ids), ptr<int64_t>(pids), ptr<int64_t>(tids), ptr<uint16_t>(ww), ptr<uint16_t>(wp),
               ptr<uint16_t>(wt), ptr<float>(gamma), ptr<float>(beta), ptr<uint16_t>(y), ptr<float>(mean), ptr<float>(rstd),
               (int)d.T, (int)d.H, (float)eps, (float)p, u32(seed), u32(opid), (int)d.V, (int)d.P, (int)d.NT, cur_stream());
  return {y, mean, rstd};
}

std::vector<Tensor> f32_embed_fwd(Tensor ids, Tensor pids, Tensor tids, Tensor ww, Tensor wp, Tensor wt, Tensor gamma,
                                  Tensor beta, double eps, double p, int64_t seed, int64_t opid) {
  const Op c("f32_embed_fwd", ids);
  const EmbDims d = embed_operands(c, F32, ids, pids, tids, ww, wp, wt, gamma);
  c.holds(beta, F32, "beta", d.H);
  c10::DeviceGuard g(c.dev);
  auto y = at::empty({d.T, d.H}, ww.options());
  auto mean = at::empty({d.T}, ww.options());
  auto rstd = at::empty({d.T}, ww.options());
  hq_f32_embed_fwd(ptr<int64_t>(ids), ptr<int64_t>(pids), ptr<int64_t>(tids), ptr<float>(ww), ptr<float>(wp), ptr<float>(wt),
                   ptr<float>(gamma), ptr<float>(beta), ptr<float>(y), ptr<float>(mean), ptr<float>(rstd), (int)d.T, (int)d.H,
                   (float)eps, (float)p, u32(seed), u32(opid), (int)d.V, (int)d.P, (int)d.NT, cur_stream());
  return {y, mean, rstd};
}

// Scratch of the sorted-run table gradients (embed_bwd, f32_embed_bwd): the (key, row) pairs and their sorted copies,
// sort_bytes of digit histograms, `chunks` pairs of carry rows.  The tensors own what `sc` points into.
struct EmbScratch { Tensor pairs, sort_tmp, carry; HqEmbScratch sc{}; };
EmbScratch emb_scratch(const Tensor& ids, const at::TensorOptions& f32, int64_t T, int64_t H, size_t sort_bytes,
                       int64_t chunks, float* ppart) {
  EmbScratch e;
  e.pairs = at::empty({4, T}, ids.options().dtype(I32));
  e.sort_tmp = at::empty({(int64_t)std::max<size_t>(sort_bytes, 1)}, ids.options().dtype(at::kByte));
  e.carry = at::empty({chunks * 2, H}, f32);
  int32_t* pr = e.pairs.data_ptr<int32_t>();
  e.sc = HqEmbScratch{pr, pr + T, pr + 2 * T, pr + 3 * T, e.sort_tmp.data_ptr(), sort_bytes, ptr<float>(e.carry), ppart};
  return e;
}

// deterministic: with more than 2 types the type gradients come from sorted runs instead of atomics;
// det_positions: so do ALL position gradients (for position ids that are not each row's column index — the
// caller knows, the host never looks at the ids).  Both off: the default paths, unchanged.
void embed_bwd(Tensor dy, Tensor ids, Tensor pids, Tensor tids, Tensor ww, Tensor wp, Tensor wt, Tensor gamma, Tensor mean,
               Tensor rstd, double p, int64_t seed, int64_t opid, Tensor g_word, Tensor g_pos, Tensor g_type, Tensor g_gamma,
               Tensor g_beta, bool accumulate, int64_t pad_word, int64_t pad_pos, int64_t seq_len, bool deterministic,
               bool det_positions) {
  const Op c("embed_bwd", dy);
  const EmbDims d = embed_bwd_operands(c, BF16, dy, ids, pids, tids, ww, wp, wt, gamma, mean, rstd, g_word, g_pos, g_type,
                                       g_gamma, g_beta);
  const int64_t T = d.T, H = d.H;
  const int V = (int)d.V, P = (int)d.P, n_types = (int)d.NT;
  c10::DeviceGuard g(c.dev);
  auto s = cur_stream();
  if (!accumulate) {
    hq_zero_f32(ptr<float>(g_word), (size_t)g_word.numel(), s);
    hq_zero_f32(ptr<float>(g_pos), (size_t)g_pos.numel(), s);
    if (n_types > 2) hq_zero_f32(ptr<float>(g_type), (size_t)g_type.numel(), s);
  }
  const int nb = hq_embed_bwd_partials((int)T, (int)seq_len);
  auto part = at::empty({nb, 4 * H}, gamma.options());
  const HqEmbScratchSizes zs = hq_embed_bwd_scratch((int)T, V, (int)seq_len, P);
  // the position / type sorts of the deterministic modes reuse the word sort's scratch: room for the largest
  size_t sort_bytes = zs.sort_bytes;
  if (det_positions) sort_bytes = std::max(sort_bytes, hq_sort_ids_bytes((int)T, P));
  if (deterministic && n_types > 2) sort_bytes = std::max(sort_bytes, hq_sort_ids_bytes((int)T, n_types));
  auto ppart = at::empty({std::max<int64_t>(det_positions ? 0 : zs.pos_rows, 1), H}, gamma.options());
  const EmbScratch es = emb_scratch(ids, gamma.options(), T, H, sort_bytes, zs.chunks, ptr<float>(ppart));
  float* t0 = ptr<float>(g_type);
  HqOuts o = outs4(ptr<float>(g_gamma), ptr<float>(g_beta), n_types <= 2 ? t0 : nullptr,
                   n_types == 2 ? t0 + H : nullptr);
  hq_embed_bwd(ptr<uint16_t>(dy), ptr<int64_t>(ids), ptr<int64_t>(pids), ptr<int64_t>(tids), ptr<uint16_t>(ww),
               ptr<uint16_t>(wp), ptr<uint16_t>(wt), ptr<float>(gamma), ptr<float>(mean), ptr<float>(rstd),
               ptr<float>(g_word), ptr<float>(g_pos), t0, ptr<float>(part), o, (int)T, (int)H, n_types, (int)pad_word,
               (int)pad_pos, (float)p, u32(seed), u32(opid), accumulate, V, P, (int)seq_len, es.sc, s, det_positions,
               deterministic);
}

void f32_embed_bwd(Tensor dy, Tensor ids, Tensor pids, Tensor tids, Tensor ww, Tensor wp, Tensor wt, Tensor gamma, Tensor mean,
                   Tensor rstd, double p, int64_t seed, int64_t opid, Tensor g_word, Tensor g_pos, Tensor g_type,
                   Tensor g_gamma, Tensor g_beta, bool accumulate, int64_t pad_word, int64_t pad_pos, bool deterministic) {
  const Op c("f32_embed_bwd", dy);
  const EmbDims d = embed_bwd_operands(c, F32, dy, ids, pids, tids, ww, wp, wt, gamma, mean, rstd, g_word, g_pos, g_type,
                                       g_gamma, g_beta);
  const int64_t T = d.T, H = d.H;
  const int V = (int)d.V, P = (int)d.P, n_types = (int)d.NT;
  c10::DeviceGuard g(c.dev);
  auto s = cur_stream();
  if (!accumulate) {
    hq_zero_f32(ptr<float>(g_word), (size_t)g_word.numel(), s);
    hq_zero_f32(ptr<float>(g_pos), (size_t)g_pos.numel(), s);
    if (n_types > 2) hq_zero_f32(ptr<float>(g_type), (size_t)g_type.numel(), s);   // else folded from partials
  }
  auto part = at::empty({hq_f32_part_rows((int)T), 4 * H}, dy.options());
  // deterministic: per-call scratch of the sorted-run path (sort pairs, digit histograms of the widest key, carry
  // rows), shared by the word, position and type passes
  EmbScratch es;
  if (deterministic) {
    size_t sort_bytes = std::max(hq_sort_ids_bytes((int)T, V), hq_sort_ids_bytes((int)T, P));
    if (n_types > 2) sort_bytes = std::max(sort_bytes, hq_sort_ids_bytes((int)T, n_types));
    es = emb_scratch(ids, dy.options(), T, H, sort_bytes, std::max(hq_emb_run_chunks((int)T), 1), nullptr);
  }
  float* t0 = ptr<float>(g_type);
  hq_f32_embed_bwd(ptr<float>(dy), ptr<int64_t>(ids), ptr<int64_t>(pids), ptr<int64_t>(tids), ptr<float>(ww), ptr<float>(wp),
                   ptr<float>(wt), ptr<float>(gamma), ptr<float>(mean), ptr<float>(rstd), ptr<float>(g_word),
                   ptr<float>(g_pos), t0, ptr<float>(part),
                   outs4(ptr<float>(g_gamma), ptr<float>(g_beta), n_types <= 2 ? t0 : nullptr, n_types == 2 ? t0 + H : nullptr),
                   (int)T, (int)H, (int)pad_word, (int)pad_pos, (float)p, u32(seed), u32(opid), accumulate, V, P, n_types, s,
                   deterministic ? &es.sc : nullptr);
}

// ------------------------------------------------- attention_fwd.hip, attention_bwd.hip, f32_attention.hip
// Forward and backward of both precisions: qkv [B·L, 3·nh·64] of `dt`, key_bias f32 with B·L elements; one workgroup
// row per (batch, head); the 32-bit element index of the dropout stream.  Returns H = nh·64.
int64_t attn_operands(const Op& c, at::ScalarType dt, const Tensor& qkv, const Tensor& key_bias, int64_t B, int64_t L,
                      int64_t nh) {
  TORCH_CHECK(B >= 1 && L >= 1 && nh >= 1 && B * nh < 65536, c.op, ": B, L, nh are ", B, ", ", L, ", ", nh,
              ", expected all >= 1 and B*nh < 65536 (grid limit)");
  TORCH_CHECK(B * nh * L * L < kU32Max, c.op, ": B*nh*L*L is ", B * nh * L * L, ", expected to fit the 32-bit dropout index");
  c.is(qkv, dt, "qkv", {B * L, 3 * nh * 64});   // head_dim 64
  c.holds(key_bias, F32, "key_bias", B * L);
  return nh * 64;
}

// + the backward's own: dctx, ctx [B·L, H] of `dt`, lse f32 with B·nh·L elements
int64_t attn_bwd_operands(const Op& c, at::ScalarType dt, const Tensor& dctx, const Tensor& qkv, const Tensor& ctx,
                          const Tensor& lse, const Tensor& key_bias, int64_t B, int64_t L, int64_t nh) {
  const int64_t H = attn_operands(c, dt, qkv, key_bias, B, L, nh);
  c.is(dctx, dt, "dctx", {B * L, H});
  c.is(ctx, dt, "ctx", {B * L, H});
  c.holds(lse, F32, "lse", B * nh * L);
  return H;
}

std::vector<Tensor> attn_fwd(Tensor qkv, Tensor key_bias, int64_t B, int64_t L, int64_t nh, double p, int64_t seed,
                             int64_t opid, double scale, OptTensor q8, int64_t phase) {
  const Op c("attn_fwd", qkv);
  const int64_t H = attn_operands(c, BF16, qkv, key_bias, B, L, nh);
  const bool want8 = has(q8);
  float* q8p = c.state4(q8, "q8");
  c10::DeviceGuard g(c.dev);
  auto ctx = at::empty({B * L, H}, qkv.options());
  auto lse = at::empty({B, nh, L}, key_bias.options());
  const int64_t mbytes = p > 0 ? (int64_t)hq_attn_mask_bytes((int)B, (int)L, (int)nh) : 0;
  auto mbits = at::empty({mbytes / 2}, qkv.options().dtype(at::kShort));
  Tensor ctx8 = want8 ? at::empty({B * L, H}, qkv.options().dtype(E4M3)) : Tensor();
  hq_attn_fwd(ptr<uint16_t>(qkv), ptr<float>(key_bias), ptr<uint16_t>(ctx), ptr<float>(lse),
              mbytes ? ptr<uint16_t>(mbits) : nullptr, (int)B, (int)L, (int)nh, 64, (float)p, u32(seed), u32(opid),
              (float)scale, cur_stream(), want8 ? reinterpret_cast<uint8_t*>(ctx8.data_ptr()) : nullptr, q8p,
              (int)(phase % 3));
  if (want8) return {ctx, lse, mbits, ctx8};
  return {ctx, lse, mbits};
}

std::vector<Tensor> f32_attn_fwd(Tensor qkv, Tensor key_bias, int64_t B, int64_t L, int64_t nh, double p, int64_t seed,
                                 int64_t opid, double scale) {
  const Op c("f32_attn_fwd", qkv);
  const int64_t H = attn_operands(c, F32, qkv, key_bias, B, L, nh);
  c10::DeviceGuard g(c.dev);
  auto ctx = at::empty({B * L, H}, qkv.options());
  auto lse = at::empty({B, nh, L}, qkv.options());
  hq_f32_attn_fwd(ptr<float>(qkv), ptr<float>(key_bias), ptr<float>(ctx), ptr<float>(lse), (int)B, (int)L, (int)nh, (float)p,
                  u32(seed), u32(opid), (float)scale, cur_stream());
  return {ctx, lse};
}

// q8 given (--precision fp8): also dQKV as e5m2 under that delayed-scaling state -> [dqkv, dqkv8]; with
// write_bf16 = false: [empty, dqkv8, bpart] — no bf16 dQKV, the QKV bias-gradient column partials
// bpart [B·ceil(L/32), 3H] instead (colsum_into reduces them).
// `deterministic` is accepted and ignored: both backward kernels are deterministic (no atomics).
std::vector<Tensor> attn_bwd_impl(const char* op, Tensor dctx, Tensor qkv, Tensor ctx, Tensor lse, Tensor key_bias,
                                  Tensor mbits, int64_t B, int64_t L, int64_t nh, double p, double scale, OptTensor q8,
                                  int64_t phase, bool write_bf16) {
  const Op c(op, dctx);
  attn_bwd_operands(c, BF16, dctx, qkv, ctx, lse, key_bias, B, L, nh);
  if (p > 0) c.holds(mbits, at::kShort, "mbits", (int64_t)hq_attn_mask_bytes((int)B, (int)L, (int)nh) / 2);
  const bool want8 = has(q8);
  TORCH_CHECK(write_bf16 || want8, op, ": write_bf16=False needs q8");
  float* q8p = c.state4(q8, "q8");
  c10::DeviceGuard g(c.dev);
  auto dqkv = write_bf16 ? at::empty_like(qkv) : at::empty({0}, qkv.options());
  auto delta = at::empty({B, nh, L}, lse.options());
  Tensor bpart = write_bf16 ? Tensor() : at::empty({B * ((L + 31) / 32), qkv.size(1)}, lse.options());
  Tensor dqkv8 = want8 ? at::empty(qkv.sizes(), qkv.options().dtype(E5M2)) : Tensor();
  hq_attn_bwd(ptr<uint16_t>(dctx), ptr<uint16_t>(qkv), ptr<uint16_t>(ctx), ptr<float>(lse), ptr<float>(key_bias),
              p > 0 ? ptr<uint16_t>(mbits) : nullptr, write_bf16 ? ptr<uint16_t>(dqkv) : nullptr, ptr<float>(delta), (int)B,
              (int)L, (int)nh, 64, (float)p, (float)scale, cur_stream(),
              want8 ? reinterpret_cast<uint8_t*>(dqkv8.data_ptr()) : nullptr, q8p, (int)(phase % 3),
              write_bf16 ? nullptr : ptr<float>(bpart));
  if (!write_bf16) return {dqkv, dqkv8, bpart};
  if (want8) return {dqkv, dqkv8};
  return {dqkv};
}

Tensor attn_bwd(Tensor dctx, Tensor qkv, Tensor ctx, Tensor lse, Tensor key_bias, Tensor mbits, int64_t B, int64_t L,
                int64_t nh, double p, double scale, bool /*deterministic*/) {
  return attn_bwd_impl("attn_bwd", dctx, qkv, ctx, lse, key_bias, mbits, B, L, nh, p, scale, c10::nullopt, 0, true)[0];
}

std::vector<Tensor> attn_bwd_q8(Tensor dctx, Tensor qkv, Tensor ctx, Tensor lse, Tensor key_bias, Tensor mbits, int64_t B,
                                int64_t L, int64_t nh, double p, double scale, bool /*deterministic*/, Tensor q8,
                                int64_t phase, bool write_bf16) {
  return attn_bwd_impl("attn_bwd_q8", dctx, qkv, ctx, lse, key_bias, mbits, B, L, nh, p, scale, q8, phase, write_bf16);
}

Tensor f32_attn_bwd(Tensor dctx, Tensor qkv, Tensor ctx, Tensor lse, Tensor key_bias, int64_t B, int64_t L, int64_t nh,
                    double p, int64_t seed, int64_t opid, double scale) {
  const Op c("f32_attn_bwd", dctx);
  attn_bwd_operands(c, F32, dctx, qkv, ctx, lse, key_bias, B, L, nh);
  c10::DeviceGuard g(c.dev);
  auto dqkv = at::empty_like(qkv);
  auto delta = at::empty({B, nh, L}, qkv.options());
  hq_f32_attn_bwd(ptr<float>(dctx), ptr<float>(qkv), ptr<float>(ctx), ptr<float>(lse), ptr<float>(key_bias), ptr<float>(dqkv),
                  ptr<float>(delta), (int)B, (int)L, (int)nh, (float)p, u32(seed), u32(opid), (float)scale, cur_stream());
  return dqkv;
}

// ------------------------------------------------------------------------------------ optim.hip
std::vector<Tensor> grad_norm(Tensor grad, double max_norm) {
  const Op c("grad_norm", grad);
  c.dense(grad, F32, "grad");
  c10::DeviceGuard g(c.dev);
  const int nparts = 1024;
  auto part = at::empty({nparts}, grad.options());
  auto norm = at::empty({1}, grad.options());
  auto coef = at::empty({1}, grad.options());
  auto s = cur_stream();
  hq_sq_norm_partials(ptr<float>(grad), grad.numel(), ptr<float>(part), nparts, s);
  hq_clip_coef(ptr<float>(part), nparts, (float)max_norm, ptr<float>(norm), ptr<float>(coef), s);
  return {norm, coef};
}

Tensor sq_norm_partials(Tensor x, int64_t nparts) {
  const Op c("sq_norm_partials", x);
  c.dense(x, F32, "x");
  c10::DeviceGuard g(c.dev);
  auto part = at::empty({nparts}, x.options());
  hq_sq_norm_partials(ptr<float>(x), x.numel(), ptr<float>(part), (int)nparts, cur_stream());
  return part;
}

Tensor fingerprint(Tensor x, int64_t nparts) {
  const Op c("fingerprint", x);
  c.dense(x, F32, "x");
  TORCH_CHECK(nparts > 0 && nparts <= 65535, "fingerprint: nparts is ", nparts, ", expected 1..65535");
  c10::DeviceGuard g(c.dev);
  auto out = at::empty({nparts}, x.options().dtype(I64));
  hq_fingerprint(ptr<float>(x), x.numel(), (int)nparts, reinterpret_cast<uint64_t*>(out.data_ptr<int64_t>()),
                 cur_stream());
  return out;
}

// the [C, 2] int64 chunk table of the optimizers and the chunked grad norm (contents trusted: built by ParamStore)
int64_t chunk_table(const Op& c, const Tensor& chunks) {
  const int64_t C = c.matrix(chunks, "chunks")[0];
  c.is(chunks, I64, "chunks", {C, 2});
  return C;
}

// grad norm over the chunk table (ParamStore.norm_chunks): partials[c0:c1] on the current stream
void sq_norm_chunks(Tensor grad, Tensor chunks, int64_t c0, int64_t c1, Tensor partials) {
  const Op c("sq_norm_chunks", grad);
  c.dense(grad, F32, "grad");
  const int64_t C = chunk_table(c, chunks);
  c.holds(partials, F32, "partials", C);
  TORCH_CHECK(0 <= c0 && c0 <= c1 && c1 <= C, "sq_norm_chunks: chunk range is [", c0, ", ", c1, "), expected within [0, ", C,
              "]");
  c10::DeviceGuard g(c.dev);
  hq_sq_norm_chunks(ptr<float>(grad), ptr<int64_t>(chunks), (int)c0, (int)c1, ptr<float>(partials), cur_stream());
}

// (norm, coef) from a complete partials vector (deterministic fixed-order sum)
std::vector<Tensor> clip_from_partials(Tensor partials, double max_norm) {
  const Op c("clip_from_partials", partials);
  c.dense(partials, F32, "partials");
  c10::DeviceGuard g(c.dev);
  auto norm = at::empty({1}, partials.options());
  auto coef = at::empty({1}, partials.options());
  hq_clip_coef(ptr<float>(partials), (int)partials.numel(), (float)max_norm, ptr<float>(norm), ptr<float>(coef),
               cur_stream());
  return {norm, coef};
}

HqOptGroups groups_of(const std::vector<double>& lr, const std::vector<double>& wd) {
  TORCH_CHECK(lr.size() == wd.size() && lr.size() <= (size_t)kOptMaxGroups, "at most 8 param groups");
  HqOptGroups gr{};
  for (size_t i = 0; i < lr.size(); ++i) { gr.lr[i] = (float)lr[i]; gr.wd[i] = (float)wd[i]; }
  return gr;
}

void adamw(Tensor master, OptTensor compute, Tensor grad, Tensor m, Tensor v, Tensor chunks, std::vector<double> lr,
           std::vector<double> wd, double beta1, double beta2, double eps, double step_mult, OptTensor clip_coef) {
  const Op c("adamw", master);
  const int64_t n = master.numel();
  c.dense(master, F32, "master");
  c.holds(compute, BF16, "compute", n);
  c.holds(grad, F32, "grad", n);
  c.holds(m, F32, "exp_avg", n);
  c.holds(v, F32, "exp_avg_sq", n);
  const int64_t C = chunk_table(c, chunks);
  if (has(clip_coef)) c.at_least(*clip_coef, F32, "clip_coef", 1);
  c10::DeviceGuard g(c.dev);
  hq_adamw(ptr<float>(master), optr<uint16_t>(compute), ptr<float>(grad), ptr<float>(m), ptr<float>(v),
           reinterpret_cast<const HqOptChunk*>(chunks.data_ptr()), (int)C, groups_of(lr, wd), HqBeta(beta1),
           HqBeta(beta2), (float)eps, (float)step_mult, optr<float>(clip_coef), cur_stream());
}

void adamod(Tensor master, OptTensor compute, Tensor grad, Tensor m, Tensor v, Tensor n_, Tensor chunks,
            std::vector<double> lr, std::vector<double> wd, double beta1, double beta2, double beta3, double eps,
            double bias_corr, OptTensor clip_coef) {
  const Op c("adamod", master);
  const int64_t n = master.numel();
  c.dense(master, F32, "master");
  c.holds(compute, BF16, "compute", n);
  c.holds(grad, F32, "grad", n);
  c.holds(m, F32, "exp_avg", n);
  c.holds(v, F32, "exp_avg_sq", n);
  c.holds(n_, F32, "exp_avg_lr", n);
  const int64_t C = chunk_table(c, chunks);
  if (has(clip_coef)) c.at_least(*clip_coef, F32, "clip_coef", 1);
  c10::DeviceGuard g(c.dev);
  hq_adamod(ptr<float>(master), optr<uint16_t>(compute), ptr<float>(grad), ptr<float>(m), ptr<float>(v), ptr<float>(n_),
            reinterpret_cast<const HqOptChunk*>(chunks.data_ptr()), (int)C, groups_of(lr, wd), HqBeta(beta1),
            HqBeta(beta2), HqBeta(beta3), (float)eps, (float)bias_corr, optr<float>(clip_coef), cur_stream());
}

// LAMB.  The kernels trust their tables, so the tables are checked ONCE, on the host, where they are built:
// lamb_plan takes the chunk table and seg_first_chunk as CPU tensors, validates every row against the arena, derives
// the per-chunk segment index and uploads all three.  The step bindings accept only such a plan and check the arenas
// against it, so a bad table or shape raises before any launch and a step never reads a table back.
struct LambPlan {
  Tensor chunks, seg_first_chunk, chunk_seg;   // device: int64 [nchunks,2], int32 [nseg+1], int32 [nchunks]
  int64_t arena_numel = 0;
  int64_t nchunks = 0, nseg = 0, ngroups = 0;
};

LambPlan lamb_plan(Tensor master, Tensor chunks, Tensor seg_first_chunk) {
  const Op c("lamb_plan", master);
  c.dense(master, F32, "master");
  TORCH_CHECK(!chunks.is_cuda() && chunks.scalar_type() == I64 && chunks.is_contiguous() && chunks.dim() == 2 &&
                  chunks.size(1) == 2, "chunks must be a CPU [n,2] int64 tensor");
  TORCH_CHECK(!seg_first_chunk.is_cuda() && seg_first_chunk.scalar_type() == I32 && seg_first_chunk.is_contiguous() &&
                  seg_first_chunk.dim() == 1, "seg_first_chunk must be a CPU int32 vector");
  const int64_t nc = chunks.size(0), ns = seg_first_chunk.size(0) - 1, N = master.numel();
  TORCH_CHECK(nc >= 1 && nc < (int64_t)std::numeric_limits<int32_t>::max() / 2, "chunk count");
  TORCH_CHECK(ns >= 1 && ns <= nc, "seg_first_chunk must have nseg + 1 entries, 1 <= nseg <= nchunks");
  const auto* ch = reinterpret_cast<const HqOptChunk*>(chunks.data_ptr());
  const int32_t* first = seg_first_chunk.data_ptr<int32_t>();
  TORCH_CHECK(first[0] == 0 && first[ns] == nc, "seg_first_chunk does not match the chunk table: must run from 0 to nchunks");
  auto chunk_seg = at::empty({nc}, seg_first_chunk.options());
  int32_t* cs = chunk_seg.data_ptr<int32_t>();
  int64_t ngroups = 0, prev_end = 0;
  for (int64_t s = 0; s < ns; ++s) {
    TORCH_CHECK(first[s] < first[s + 1] && first[s + 1] <= nc, "seg_first_chunk does not match the chunk table: segment ", s,
                " is empty or out of range");
    for (int64_t i = first[s]; i < first[s + 1]; ++i) {
      TORCH_CHECK(ch[i].group >= 0 && ch[i].group < kOptMaxGroups, "chunk ", i, ": group index ", ch[i].group, " >= ",
                  kOptMaxGroups);
      TORCH_CHECK(ch[i].numel >= 1 && ch[i].numel <= kOptChunk, "chunk ", i, ": numel ", ch[i].numel);
      TORCH_CHECK(ch[i].start >= prev_end && ch[i].start <= N - ch[i].numel, "chunk ", i, " [", ch[i].start, ", +",
                  ch[i].numel, ") overlaps its predecessor or lies outside the arena of ", N);
      if (i > first[s])
        TORCH_CHECK(ch[i].start == prev_end && ch[i].group == ch[i - 1].group, "seg_first_chunk does not match the chunk "
                    "table: chunk ", i, " does not continue segment ", s);
      prev_end = ch[i].start + ch[i].numel;
      ngroups = std::max<int64_t>(ngroups, ch[i].group + 1);
      cs[i] = (int32_t)s;
    }
  }
  LambPlan p;
  p.chunks = chunks.to(master.device());
  p.seg_first_chunk = seg_first_chunk.to(master.device());
  p.chunk_seg = chunk_seg.to(master.device());
  p.arena_numel = N; p.nchunks = nc; p.nseg = ns; p.ngroups = ngroups;
  return p;
}

HqLambGroups lamb_groups(const LambPlan& plan, const std::vector<double>& lr, const std::vector<double>& wd,
                         const std::vector<bool>& adapt) {
  TORCH_CHECK(lr.size() == wd.size() && lr.size() == adapt.size() && lr.size() <= (size_t)kOptMaxGroups,
              "at most 8 param groups, lr / wd / adapt of one length");
  TORCH_CHECK((int64_t)lr.size() >= plan.ngroups, "the chunk table uses ", plan.ngroups, " groups, got ", lr.size());
  HqLambGroups gr{};
  for (size_t i = 0; i < lr.size(); ++i) { gr.lr[i] = (float)lr[i]; gr.wd[i] = (float)wd[i]; gr.adapt[i] = adapt[i] ? 1 : 0; }
  return gr;
}

// A LAMB binding's Op is built on the plan's own chunk table, so "the first operand's device" is the plan's.
void lamb_arena(const Op& c, const LambPlan& plan, const Tensor& t, at::ScalarType dt, const char* name) {
  c.dense(t, dt, name);
  TORCH_CHECK(t.numel() == plan.arena_numel, c.op, ": ", name, " has ", t.numel(), " elements, expected ", plan.arena_numel,
              " (the plan was made for that arena)");
}
void lamb_scratch(const Op& c, const LambPlan& plan, const Tensor& partials, const Tensor& norms) {
  c.holds(partials, F32, "partials", 2 * plan.nchunks);   // [nchunks, 2]
  c.holds(norms, F32, "norms", 3 * plan.nseg);            // [nseg, 3]
}

// bc1 = 1/(1 − β1^t), bc2 = 1/(1 − β2^t) (or 1): doubles from the caller, rounded once here
void lamb_moments(const LambPlan& plan, Tensor master, Tensor grad, Tensor m, Tensor v, std::vector<double> lr,
                  std::vector<double> wd, std::vector<bool> adapt, double beta1, double beta2, double eps, double bc1,
                  double bc2, OptTensor clip_coef, Tensor partials, Tensor norms) {
  const Op c("lamb_moments", plan.chunks);
  lamb_arena(c, plan, master, F32, "master");
  lamb_arena(c, plan, grad, F32, "grad");
  lamb_arena(c, plan, m, F32, "exp_avg");
  lamb_arena(c, plan, v, F32, "exp_avg_sq");
  if (has(clip_coef)) c.at_least(*clip_coef, F32, "clip_coef", 1);
  lamb_scratch(c, plan, partials, norms);
  const HqLambGroups gr = lamb_groups(plan, lr, wd, adapt);
  c10::DeviceGuard g(c.dev);
  hq_lamb_moments(ptr<float>(master), ptr<float>(grad), ptr<float>(m), ptr<float>(v),
                  reinterpret_cast<const HqOptChunk*>(plan.chunks.data_ptr()), (int)plan.nchunks, gr,
                  HqLambArgs(HqBeta(beta1), HqBeta(beta2), (float)eps, (float)bc1, (float)bc2), optr<float>(clip_coef),
                  ptr<float>(partials), cur_stream());
}

void lamb_ratio(const LambPlan& plan, std::vector<double> lr, std::vector<double> wd, std::vector<bool> adapt,
                Tensor partials, Tensor norms) {
  const Op c("lamb_ratio", plan.chunks);
  lamb_scratch(c, plan, partials, norms);
  const HqLambGroups gr = lamb_groups(plan, lr, wd, adapt);
  c10::DeviceGuard g(c.dev);
  hq_lamb_ratio(ptr<float>(partials), reinterpret_cast<const HqOptChunk*>(plan.chunks.data_ptr()),
                plan.seg_first_chunk.data_ptr<int32_t>(), (int)plan.nseg, gr, ptr<float>(norms), cur_stream());
}

void lamb_apply(const LambPlan& plan, Tensor master, OptTensor compute, Tensor m, Tensor v, std::vector<double> lr,
                std::vector<double> wd, std::vector<bool> adapt, double beta1, double beta2, double eps, double bc1,
                double bc2, Tensor partials, Tensor norms) {
  const Op c("lamb_apply", plan.chunks);
  lamb_arena(c, plan, master, F32, "master");
  if (has(compute)) lamb_arena(c, plan, *compute, BF16, "compute");
  lamb_arena(c, plan, m, F32, "exp_avg");
  lamb_arena(c, plan, v, F32, "exp_avg_sq");
  lamb_scratch(c, plan, partials, norms);
  const HqLambGroups gr = lamb_groups(plan, lr, wd, adapt);
  c10::DeviceGuard g(c.dev);
  hq_lamb_apply(ptr<float>(master), optr<uint16_t>(compute), ptr<float>(m), ptr<float>(v),
                reinterpret_cast<const HqOptChunk*>(plan.chunks.data_ptr()), plan.chunk_seg.data_ptr<int32_t>(),
                (int)plan.nchunks, gr, HqLambArgs(HqBeta(beta1), HqBeta(beta2), (float)eps, (float)bc1, (float)bc2),
                ptr<float>(norms), cur_stream());
}

// the whole step: every argument is checked before the first of the three launches
void lamb_step(const LambPlan& plan, Tensor master, OptTensor compute, Tensor grad, Tensor m, Tensor v,
               std::vector<double> lr, std::vector<double> wd, std::vector<bool> adapt, double beta1, double beta2,
               double eps, double bc1, double bc2, OptTensor clip_coef, Tensor partials, Tensor norms) {
  const Op c("lamb_step", plan.chunks);
  if (has(compute)) lamb_arena(c, plan, *compute, BF16, "compute");   // the one operand lamb_moments does not see
  lamb_moments(plan, master, grad, m, v, lr, wd, adapt, beta1, beta2, eps, bc1, bc2, clip_coef, partials, norms);
  lamb_ratio(plan, lr, wd, adapt, partials, norms);
  lamb_apply(plan, master, compute, m, v, lr, wd, adapt, beta1, beta2, eps, bc1, bc2, partials, norms);
}

void cast_f32_bf16(Tensor src, Tensor dst, double scale) {
  const Op c("cast_f32_bf16", src);
  c.dense(src, F32, "src");
  c.holds(dst, BF16, "dst", src.numel());
  c10::DeviceGuard g(c.dev);
  hq_cast_f32_bf16(ptr<float>(src), ptr<uint16_t>(dst), src.numel(), (float)scale, cur_stream());
}

void cast_bf16_f32(Tensor src, Tensor dst, double scale) {
  const Op c("cast_bf16_f32", src);
  c.dense(src, BF16, "src");
  c.holds(dst, F32, "dst", src.numel());
  c10::DeviceGuard g(c.dev);
  hq_cast_bf16_f32(ptr<uint16_t>(src), ptr<float>(dst), src.numel(), (float)scale, cur_stream());
}

// ------------------------------------------------------------------------------------ gemm_nt.hip
// C[M,N] = A[M,K] · B[N,K]^T with epilogue `epi` (HQ_EPI_*).  bias f32[N] (BIAS/GELU/GELUD/BDR); pre bf16[M,N]
// (GELU: written, DGELU: read); resid bf16[M,N] (RESID, BDR); part f32[gemm_nt_part_rows, N] (DGELU column partials).
int64_t gemm_nt_supported(int64_t M, int64_t N, int64_t K) { return hq_gemm_nt_supported((int)M, (int)N, (int)K); }
int64_t gemm_nt_part_rows(int64_t M, int64_t N, int64_t K) { return (int64_t)hq_gemm_nt_part_rows((int)M, (int)N, (int)K); }
// floats of the split-K workspace gemm_nt allocates for this shape and epilogue: ksplit·M·N, or 0 (no split)
int64_t gemm_nt_ws_floats(int64_t M, int64_t N, int64_t K, int64_t epi) {
  return (int64_t)hq_gemm_nt_ws_floats((int)M, (int)N, (int)K, (int)epi);
}

Tensor gemm_nt(Tensor A, Tensor B, int64_t epi, OptTensor bias, OptTensor pre, OptTensor resid, OptTensor part,
               OptTensor out, double p, int64_t seed, int64_t opid) {
  const Op c("gemm_nt", A);
  const auto [M, K] = c.matrix(A, "A");
  const int64_t N = c.matrix(B, "B")[0];
  c.is(A, BF16, "A", {M, K});
  c.is(B, BF16, "B", {N, K});
  TORCH_CHECK(M < (1ll << 31) / 4 && N * K < (1ll << 31) && M * N < (1ll << 40), "gemm_nt: shape too large");
  const int bn = hq_gemm_nt_supported((int)M, (int)N, (int)K);
  TORCH_CHECK(bn > 0, "gemm_nt: unsupported shape M=", M, " N=", N, " K=", K, " (need N%128, K%64 == 0)");
  TORCH_CHECK(epi >= HQ_EPI_NONE && epi <= HQ_EPI_BDR, "gemm_nt: bad epilogue");
  // which operands the epilogue dereferences: each is required, then checked like any other
  const bool col_part = hq_epi_col_partials((int)epi);
  if (epi == HQ_EPI_BDR)
    TORCH_CHECK(M * N < kU32Max, "gemm_nt: M*N exceeds 32-bit dropout index");
  if (hq_epi_has_bias((int)epi)) {
    TORCH_CHECK(has(bias), "gemm_nt: bias required");
    c.holds(bias, F32, "bias", N);
  }
  if (hq_epi_writes_p((int)epi) || col_part) {   // P written, or read as the operand
    TORCH_CHECK(has(pre), "gemm_nt: pre required");
    c.is(pre, BF16, "pre", {M, N});
  }
  if (hq_epi_reads_aux((int)epi) && !col_part) {   // the operand is R
    TORCH_CHECK(has(resid), "gemm_nt: resid required");
    c.is(resid, BF16, "resid", {M, N});
  }
  if (col_part) {
    TORCH_CHECK(has(part), "gemm_nt: part required");
    c.holds(part, F32, "part", (int64_t)hq_gemm_nt_part_rows((int)M, (int)N, (int)K) * N);   // [gemm_nt_part_rows, N]
  }
  c.is(out, BF16, "out", {M, N});
  c10::DeviceGuard g(c.dev);
  Tensor C = has(out) ? *out : at::empty({M, N}, A.options());
  // split-K slabs (128² kernel, low-fill long-K grids) from the stream-aware caching allocator: safe beside
  // other streams and inside graph captures once the shape has run eagerly
  const size_t wsf = hq_gemm_nt_ws_floats((int)M, (int)N, (int)K, (int)epi);
  Tensor ws = wsf ? at::empty({(int64_t)wsf}, A.options().dtype(F32)) : Tensor();
  hq_gemm_nt(ptr<uint16_t>(A), ptr<uint16_t>(B), ptr<uint16_t>(C), optr<float>(bias), optr<uint16_t>(pre),
             optr<uint16_t>(resid), optr<float>(part), (int)M, (int)N, (int)K, (int)K, (int)K, (int)N, (int)epi, bn,
             cur_stream(), (float)p, u32(seed), u32(opid), wsf ? ws.data_ptr<float>() : nullptr);
  return C;
}

// ------------------------------------------------------------------------------------ gemm_f32.hip
// --precision fp32: exact-f32 strided / batched GEMM.  C(z, i, j) = alpha·Σ_k A(z,i,k)·B(z,j,k) (+ bias[j])
// (+ R(z,i,j)), every operand addressed from its tensor's data_ptr by the given strides — the span check proves every
// element the grid touches lies inside its tensor's storage.
void f32_span_check(const Op& c, const Tensor& t, const char* name, std::initializer_list<std::pair<int64_t, int64_t>> dims) {
  c.on(t, F32, name);
  int64_t hi = 0;
  for (auto& d : dims) {
    TORCH_CHECK(d.first >= 1 && d.second >= 0, c.op, ": ", name, ": bad extent/stride");
    hi += (d.first - 1) * d.second;
  }
  const int64_t avail = (int64_t)(t.storage().nbytes() / 4) - t.storage_offset();
  TORCH_CHECK(hi < avail, c.op, ": ", name, ": strided extent ", hi + 1, " exceeds the tensor's storage (", avail, " floats)");
  TORCH_CHECK(((uintptr_t)t.data_ptr() & 15) == 0, c.op, ": ", name, " must be 16-byte aligned");
}

void gemm_f32(Tensor A, Tensor B, Tensor C, int64_t M, int64_t N, int64_t K, std::vector<int64_t> sa,
              std::vector<int64_t> sb, std::vector<int64_t> sc, int64_t batch, int64_t nb_in, double alpha,
              OptTensor bias, OptTensor R, int64_t ldr, const std::string& mode) {
  // sa = {sa_i, sa_k, ba_out, ba_in}, sb = {sb_j, sb_k, bb_out, bb_in}, sc = {ldc, bc_out, bc_in}
  // mode: "exact" (f32-input MFMA) or "bf16x3" (three bf16 MFMAs over a hi + mid split of each operand)
  const Op c("gemm_f32", A);
  TORCH_CHECK(mode == "exact" || mode == "bf16x3", "gemm_f32: mode must be 'exact' or 'bf16x3', got '", mode, "'");
  TORCH_CHECK(sa.size() == 4 && sb.size() == 4 && sc.size() == 3, "gemm_f32: stride vectors");
  TORCH_CHECK(M > 0 && N > 0 && K > 0 && batch >= 1 && nb_in >= 1 && batch % nb_in == 0, "gemm_f32: bad sizes");
  TORCH_CHECK(M * N < (int64_t)1 << 31 && K < (int64_t)1 << 31, "gemm_f32: sizes exceed 32-bit tile indexing");
  const int64_t nbo = batch / nb_in;
  TORCH_CHECK(sa[1] == 1 || sa[0] == 1, "gemm_f32: A needs a unit i or k stride");
  TORCH_CHECK(sb[1] == 1 || sb[0] == 1, "gemm_f32: B needs a unit j or k stride");
  // float4 staging: the contiguous extent is a multiple of 4 and the other stride keeps quads 16-B aligned
  if (sa[1] == 1) {
    TORCH_CHECK(K % 4 == 0 && sa[0] % 4 == 0, "gemm_f32: k-contiguous A needs K % 4 == 0, sa_i % 4 == 0");
  } else {
    TORCH_CHECK(M % 4 == 0 && sa[1] % 4 == 0, "gemm_f32: i-contiguous A needs M % 4 == 0, sa_k % 4 == 0");
  }
  if (sb[1] == 1) {
    TORCH_CHECK(K % 4 == 0 && sb[0] % 4 == 0, "gemm_f32: k-contiguous B needs K % 4 == 0, sb_j % 4 == 0");
  } else {
    TORCH_CHECK(N % 4 == 0 && sb[1] % 4 == 0, "gemm_f32: j-contiguous B needs N % 4 == 0, sb_k % 4 == 0");
  }
  TORCH_CHECK(sa[2] % 4 == 0 && sa[3] % 4 == 0 && sb[2] % 4 == 0 && sb[3] % 4 == 0, "gemm_f32: batch strides % 4");
  f32_span_check(c, A, "A", {{M, sa[0]}, {K, sa[1]}, {nbo, sa[2]}, {nb_in, sa[3]}});
  f32_span_check(c, B, "B", {{N, sb[0]}, {K, sb[1]}, {nbo, sb[2]}, {nb_in, sb[3]}});
  f32_span_check(c, C, "C", {{M, sc[0]}, {N, 1}, {nbo, sc[1]}, {nb_in, sc[2]}});
  if (has(R)) f32_span_check(c, *R, "R", {{M, ldr}, {N, 1}, {nbo, sc[1]}, {nb_in, sc[2]}});
  c.holds(bias, F32, "bias", N);
  c10::DeviceGuard g(c.dev);
  const int ks = hq_gemm_f32_splits((int)M, (int)N, (int)K, (int)batch);
  Tensor ws = ks > 1 ? at::empty({ks, M, N}, C.options()) : Tensor();
  const auto launch = mode == "bf16x3" ? hq_gemm_f32x3 : hq_gemm_f32;
  launch(ptr<float>(A), ptr<float>(B), ptr<float>(C), optr<float>(bias), optr<float>(R), ks > 1 ? ptr<float>(ws) : nullptr,
         (int)M, (int)N, (int)K, sa[0], sa[1], sb[0], sb[1], (int)sc[0], (int)ldr, (int)batch, (int)nb_in, sa[2], sa[3],
         sb[2], sb[3], sc[1], sc[2], (float)alpha, ks, cur_stream());
}

// ------------------------------------------------------------------------------------ gemm_tn.hip
// Weight gradient: out [N,K] f32 (+)= dyᵀ·x with dy [T,N], x [T,K] bf16; split-K slabs from the caching allocator.
int64_t gemm_tn_splits(int64_t T, int64_t N, int64_t K) { return hq_gemm_tn_splits((int)T, (int)N, (int)K); }

void gemm_tn(Tensor dy, Tensor x, Tensor out, bool accumulate, int64_t splits, OptTensor bias_out) {
  const Op c("gemm_tn", dy);
  const auto [T, N] = c.matrix(dy, "dy");
  const int64_t K = c.matrix(x, "x")[1];
  c.is(dy, BF16, "dy", {T, N});
  c.is(x, BF16, "x", {T, K});
  c.holds(out, F32, "out", N * K);
  c.holds(bias_out, F32, "bias_out", N);
  const int auto_s = hq_gemm_tn_splits((int)T, (int)N, (int)K);
  TORCH_CHECK(auto_s > 0, "gemm_tn: unsupported shape T=", T, " N=", N, " K=", K, " (need N%128, K%128 == 0, T >= 128)");
  const int S = splits > 0 ? (int)splits : auto_s;
  TORCH_CHECK((T + 63) / 64 / S >= 2, "gemm_tn: too many splits");
  const bool has_bias = has(bias_out);
  c10::DeviceGuard g(c.dev);
  Tensor part = at::empty({S, N, K}, out.options());
  Tensor bpart = has_bias ? at::empty({S, N}, out.options()) : Tensor();
  hq_gemm_tn(ptr<uint16_t>(dy), ptr<uint16_t>(x), ptr<float>(part), ptr<float>(out), has_bias ? ptr<float>(bpart) : nullptr,
             optr<float>(bias_out), (int)T, (int)N, (int)K, S, accumulate, cur_stream());
}

// fp8 weight gradient: out [N,K] f32 (+)= (dy8ᵀ·x8)·sa·sb, dy8 e5m2 [T,N], x8 e4m3 [T,K] (token-major)
int64_t gemm_tn8_splits(int64_t T, int64_t N, int64_t K) { return hq_gemm_tn8_splits((int)T, (int)N, (int)K); }

void gemm_tn8(Tensor dy8, Tensor x8, Tensor sa, Tensor sb, Tensor out, bool accumulate) {
  const Op c("gemm_tn8", dy8);
  const auto [T, N] = c.matrix(dy8, "dy8");
  const int64_t K = c.matrix(x8, "x8")[1];
  c.is(dy8, E5M2, "dy8", {T, N});
  c.is(x8, E4M3, "x8", {T, K});
  c.at_least(sa, F32, "sa", 1);
  c.at_least(sb, F32, "sb", 1);
  c.holds(out, F32, "out", N * K);
  const int S = hq_gemm_tn8_splits((int)T, (int)N, (int)K);
  TORCH_CHECK(S > 0, "gemm_tn8: unsupported shape T=", T, " N=", N, " K=", K, " (need N%128, K%128 == 0)");
  c10::DeviceGuard g(c.dev);
  Tensor part = at::empty({S, N, K}, out.options());
  hq_gemm_tn8(reinterpret_cast<const uint8_t*>(dy8.data_ptr()), reinterpret_cast<const uint8_t*>(x8.data_ptr()),
              ptr<float>(sa), ptr<float>(sb), ptr<float>(part), ptr<float>(out), (int)T, (int)N, (int)K, S, accumulate,
              cur_stream());
}

// ------------------------------------------------------------------------------------ gemm_fp8.hip
// fp8 projection GEMM, C (bf16) = A8·B8ᵀ·sa·sb (+ epilogue), B8 e4m3.  Forward (A8 e4m3): BIAS / GELUD
// (+ bias f32; GELUD returns act, writes gelu' into `pre` and, with out8/state given, act as e4m3).
// Backward dgrad (A8 e5m2): NONE / RESID / DMUL (C ⊙ pre, column sums into part [M/256, N]; with out8/state,
// C also as e5m2).  Delayed scaling: state f32[4], phase = step % 3.
int64_t gemm_fp8_supported(int64_t M, int64_t N, int64_t K) { return hq_gemm_fp8_supported((int)M, (int)N, (int)K); }

Tensor gemm_fp8(Tensor A8, Tensor B8, int64_t epi, OptTensor bias, Tensor sa, Tensor sb, OptTensor pre, OptTensor out8,
                OptTensor state, int64_t phase, OptTensor part, OptTensor resid, bool write_out) {
  const Op c("gemm_fp8", A8);
  const bool fwd = epi == HQ_EPI_BIAS || epi == HQ_EPI_GELUD;
  const bool bwd = epi == HQ_EPI_NONE || epi == HQ_EPI_DMUL || epi == HQ_EPI_RESID;
  TORCH_CHECK(fwd || bwd, "gemm_fp8: epilogue must be BIAS / GELUD (forward) or NONE / RESID / DMUL (dgrad)");
  const auto [M, K] = c.matrix(A8, "A8");
  const int64_t N = c.matrix(B8, "B8")[0];
  c.is(A8, fwd ? E4M3 : E5M2, "A8", {M, K});   // activations forward, gradients in the dgrad
  c.is(B8, E4M3, "B8", {N, K});                // weights
  c.at_least(sa, F32, "sa", 1);
  c.at_least(sb, F32, "sb", 1);
  TORCH_CHECK(hq_gemm_fp8_supported((int)M, (int)N, (int)K), "gemm_fp8: unsupported shape M=", M, " N=", N, " K=", K);
  // write_out = false (GELUD / DMUL with out8): only the fp8 copy (and P / part) — returns an empty tensor
  TORCH_CHECK(write_out || ((epi == HQ_EPI_GELUD || epi == HQ_EPI_DMUL) && has(out8)),
              "gemm_fp8: write_out=False needs a GELUD / DMUL epilogue with out8");
  uint16_t* P = nullptr;
  uint8_t* C8 = nullptr;
  float* q8 = nullptr;
  float* pp = nullptr;
  bool code8 = true;
  if (fwd) {
    TORCH_CHECK(has(bias), "gemm_fp8: forward epilogues need the fp32 bias");
    c.holds(bias, F32, "bias", N);
  }
  if (epi == HQ_EPI_DMUL) {
    TORCH_CHECK(has(part), "gemm_fp8: DMUL needs `part` [M/256, N]");
    c.holds(part, F32, "part", (M / 256) * N);
    pp = ptr<float>(*part);
  }
  if (epi == HQ_EPI_RESID) {
    TORCH_CHECK(has(resid), "gemm_fp8: RESID needs `resid`");
    c.is(resid, BF16, "resid", {M, N});
    P = ptr<uint16_t>(*resid);
  }
  if (epi == HQ_EPI_GELUD || epi == HQ_EPI_DMUL) {
    TORCH_CHECK(has(pre), "gemm_fp8: GELUD / DMUL need `pre` (gelu')");
    // gelu' travels as the 8-bit code (hq_gd_encode8, a uint8 `pre`) between the fp8 FFN1 forward and the fp8
    // FFN2 dgrad, else as bf16.  The fp8 DMUL reads only the code; the fp8 GELUD writes bf16 gelu' (beside its
    // e4m3 act) only together with the bf16 act, i.e. when the backward will run the FFN2 dgrad in bf16.
    const bool with8 = has(out8);
    code8 = pre->scalar_type() == at::kByte;
    c.is(pre, code8 ? at::kByte : BF16, "pre", {M, N});
    if (code8) {
      TORCH_CHECK(with8, "gemm_fp8: the uint8 gelu' code (gelud_code()) goes with out8");
    } else {
      TORCH_CHECK(!with8 || (epi == HQ_EPI_GELUD && write_out),
                  "gemm_fp8: a bf16 gelu' with out8 needs GELUD with write_out (fp8 DMUL reads the uint8 code)");
    }
    P = reinterpret_cast<uint16_t*>(pre->data_ptr());
    if (with8) {
      c.holds(out8, fwd ? E4M3 : E5M2, "out8", M * N);   // e4m3 act (GELUD) / e5m2 gradient (DMUL)
      TORCH_CHECK(has(state), "gemm_fp8: out8 needs the delayed-scaling state");
      C8 = reinterpret_cast<uint8_t*>(out8->data_ptr());
      q8 = c.state4(state, "state");
    }
  }
  c10::DeviceGuard g(c.dev);
  Tensor C = write_out ? at::empty({M, N}, A8.options().dtype(BF16)) : at::empty({0}, A8.options().dtype(BF16));
  hq_gemm_fp8(reinterpret_cast<const uint8_t*>(A8.data_ptr()), reinterpret_cast<const uint8_t*>(B8.data_ptr()),
              write_out ? ptr<uint16_t>(C) : nullptr,
              optr<float>(bias), P, ptr<float>(sa), ptr<float>(sb), C8, q8, (int)(phase % 3), (int)M, (int)N, (int)K,
              (int)epi, cur_stream(), pp, code8 ? 1 : 0);
  return C;
}

// ------------------------------------------------------------------------ fp8.hip: fp8 quantisation
// x (bf16, numel % 8 == 0) -> (x8 float8_e4m3fn, scale f32[1]) with x ≈ x8 · scale (current scaling)
std::vector<Tensor> fp8_quantize(Tensor x) {
  const Op c("fp8_quantize", x);
  c.dense(x, BF16, "x");
  TORCH_CHECK(x.numel() % 8 == 0, "fp8_quantize: x has ", x.numel(), " elements, expected a multiple of 8");
  c10::DeviceGuard g(c.dev);
  auto y = at::empty(x.sizes(), x.options().dtype(E4M3));
  auto amax = at::empty({1}, x.options().dtype(I32));
  auto scale = at::empty({1}, x.options().dtype(F32));
  hq_amax_bf16(ptr<uint16_t>(x), x.numel(), ptr<unsigned>(amax), cur_stream());
  hq_fp8_quant(ptr<uint16_t>(x), ptr<uint8_t>(y), x.numel(), ptr<unsigned>(amax), ptr<float>(scale), cur_stream());
  return {y, scale.squeeze(0)};
}

// x (bf16) -> e4m3 with the delayed scale of `state` (f32[4]); returns y (float8_e4m3fn); state[3] = scale
Tensor fp8_quant_delayed(Tensor x, Tensor state, int64_t phase) {
  const Op c("fp8_quant_delayed", x);
  c.dense(x, BF16, "x");
  TORCH_CHECK(x.numel() % 8 == 0, "fp8_quant_delayed: x has ", x.numel(), " elements, expected a multiple of 8");
  c.holds(state, F32, "state", 4);
  c10::DeviceGuard g(c.dev);
  auto y = at::empty(x.sizes(), x.options().dtype(E4M3));
  hq_fp8_quant_delayed(ptr<uint16_t>(x), reinterpret_cast<uint8_t*>(y.data_ptr()), x.numel(), ptr<float>(state),
                       (int)(phase % 3), cur_stream());
  return y;
}

// Quantise many bf16 segments of `x` into `y` (uint8/e4m3 buffer) in one launch, each under its own
// delayed-scaling state row of `states` [nseg, 4].  seg: int64 [nseg, 4] = (x offset, y offset, n8,
// first block); `blocks` = total blocks (last segment's first block + its block count).  The rows of seg are
// trusted (built with the buffers by ParamStore).
void fp8_quant_delayed_multi(Tensor x, Tensor y, Tensor seg, Tensor states, int64_t blocks, int64_t phase) {
  const Op c("fp8_quant_delayed_multi", x);
  const int64_t n = c.matrix(seg, "seg")[0];
  c.dense(x, BF16, "x");
  c.dense(y, byte_dtype(y), "y");
  c.is(seg, I64, "seg", {n, 4});
  c.holds(states, F32, "states", n * 4);
  c10::DeviceGuard g(c.dev);
  hq_fp8_quant_delayed_multi(ptr<uint16_t>(x), reinterpret_cast<uint8_t*>(y.data_ptr()),
                             reinterpret_cast<const long long*>(seg.data_ptr<int64_t>()), (int)n, blocks, ptr<float>(states),
                             (int)(phase % 3), cur_stream());
}

int64_t fp8_quant_multi_blocks(int64_t n8) { return hq_fp8_quant_multi_blocks(n8); }

// bf16 gelu' -> its 8-bit code (gelud_code)
Tensor gelud_encode8(Tensor gd) {
  const Op c("gelud_encode8", gd);
  c.dense(gd, BF16, "g");
  TORCH_CHECK(gd.numel() % 8 == 0, "gelud_encode8: g has ", gd.numel(), " elements, expected a multiple of 8");
  c10::DeviceGuard g(c.dev);
  auto q = at::empty(gd.sizes(), gd.options().dtype(at::kByte));
  hq_gelud_encode8(ptr<uint16_t>(gd), q.data_ptr<uint8_t>(), gd.numel(), cur_stream());
  return q;
}

// ------------------------------------------------------------------------------------ transpose.hip
// tiles: int32 [n, 6] rows of (src_off, dst_off, rows, cols, r0, c0), trusted (built with src / dst by ParamStore)
int64_t tile_table(const Op& c, const Tensor& tiles) {
  const int64_t n = c.matrix(tiles, "tiles")[0];
  c.is(tiles, I32, "tiles", {n, 6});
  return n;
}

void transpose_tiles(Tensor src, Tensor dst, Tensor tiles) {
  const Op c("transpose_tiles", src);
  c.dense(src, BF16, "src");
  c.dense(dst, BF16, "dst");
  const int64_t n = tile_table(c, tiles);
  c10::DeviceGuard g(c.dev);
  hq_transpose_tiles(ptr<uint16_t>(src), ptr<uint16_t>(dst), ptr<int>(tiles), (int)n, cur_stream());
}

// fp8 weights (1-byte elements): the e4m3 Wᵀ copies for the fp8 dgrad GEMMs
void transpose_tiles8(Tensor src, Tensor dst, Tensor tiles) {
  const Op c("transpose_tiles8", src);
  c.dense(src, byte_dtype(src), "src");
  c.dense(dst, byte_dtype(dst), "dst");
  const int64_t n = tile_table(c, tiles);
  c10::DeviceGuard g(c.dev);
  hq_transpose_tiles8(reinterpret_cast<const uint8_t*>(src.data_ptr()), reinterpret_cast<uint8_t*>(dst.data_ptr()),
                      ptr<int>(tiles), (int)n, cur_stream());
}

// ------------------------------------------------------------------ heads.hip: the span head alone ...
// span_fwd / span_bwd: seq bf16 [..., H] (T = its rows), w f32 with 2·H elements
struct SpanDims { int64_t T, H; };
SpanDims span_operands(const Op& c, const Tensor& seq, const Tensor& w) {
  TORCH_CHECK(seq.dim() >= 1 && seq.size(-1) >= 1, c.op, ": seq has sizes ", seq.sizes(), ", expected [..., H]");
  const int64_t H = seq.size(-1), T = seq.numel() / H;
  c.dense(seq, BF16, "seq");
  c.holds(w, F32, "w", 2 * H);
  TORCH_CHECK(H % 4 == 0 && H <= 2048, c.op, ": hidden size is ", H, ", expected a multiple of 4 and <= 2048");
  return {T, H};
}

// logits [T,2] fp32 = seq[T,H] (bf16) · w[2,H]^T + b
Tensor span_fwd(Tensor seq, Tensor w, Tensor b) {
  const Op c("span_fwd", seq);
  const auto [T, H] = span_operands(c, seq, w);
  c.holds(b, F32, "b", 2);
  c10::DeviceGuard g(c.dev);
  auto logits = at::empty({T, 2}, w.options());
  hq_span_fwd(ptr<uint16_t>(seq), ptr<float>(w), ptr<float>(b), ptr<float>(logits), (int)T, (int)H, cur_stream());
  return logits;
}

// returns dseq (bf16, seq's shape); dw [2,H] f32 written (or accumulated)
Tensor span_bwd(Tensor seq, Tensor w, Tensor glog, Tensor dw, bool accumulate) {
  const Op c("span_bwd", seq);
  const auto [T, H] = span_operands(c, seq, w);
  c.holds(glog, F32, "grad_logits", 2 * T);
  c.holds(dw, F32, "dw", 2 * H);
  c10::DeviceGuard g(c.dev);
  auto dseq = at::empty_like(seq);
  auto part = at::empty({(int64_t)hq_ln_bwd_partials((int)T), 2 * H}, w.options());
  hq_span_bwd(ptr<uint16_t>(seq), ptr<float>(w), ptr<float>(glog), ptr<uint16_t>(dseq), ptr<float>(part), ptr<float>(dw),
              (int)T, (int)H, accumulate, cur_stream());
  return dseq;
}

// ------------------------------------------------------------------ ... and the fused QA heads + losses
// Ticket words of the in-launch hand-offs (heads.hip), one zeroed int32[4] per (device, stream): [0] fwd,
// [1] loss.  The last-arriving block resets its word, so a buffer is zeroed exactly once.
unsigned* ticket(const Tensor& like, int slot) {
  static std::map<std::pair<int, hipStream_t>, Tensor> words;
  const auto key = std::make_pair((int)like.get_device(), cur_stream());
  auto it = words.find(key);
  if (it == words.end()) it = words.emplace(key, at::zeros({4}, like.options().dtype(I32))).first;
  return reinterpret_cast<unsigned*>(it->second.data_ptr<int>()) + slot;
}

// qa_heads_fwd / qa_heads_bwd: seq bf16 or fp32 [..., H] with B·L rows; the ten head tensors (weights, or their
// gradients) f32: pooler [H,H] [H], classifier [NL,H] [NL], reg start / end [H] [1], span [2,H] [2]
struct HeadDims { int64_t T, B, H, NL; };
HeadDims heads_operands(const Op& c, const Tensor& seq, int64_t L, const std::vector<Tensor>& w) {
  TORCH_CHECK(w.size() == 10, c.op, ": got ", w.size(), " head weights, expected 10 (wp, bp, wc, bc, wrs, brs, wre, bre, "
              "wsp, bsp)");
  TORCH_CHECK(seq.dim() >= 1 && seq.size(-1) >= 1, c.op, ": seq has sizes ", seq.sizes(), ", expected [..., H]");
  const int64_t H = seq.size(-1), T = seq.numel() / H, NL = w[3].numel();
  c.dense(seq, seq.scalar_type() == F32 ? F32 : BF16, "seq");
  TORCH_CHECK(L > 0 && T % L == 0, c.op, ": seq has ", T, " rows, expected a multiple of L = ", L);
  TORCH_CHECK(H % 64 == 0 && H <= 2048, "fused heads need hidden % 64 == 0 and <= 2048, got ", H);
  TORCH_CHECK(NL >= 1 && NL <= 8, "fused heads support 1..8 classes, got ", NL);
  TORCH_CHECK(T * H < (int64_t)std::numeric_limits<int32_t>::max(), c.op, ": T*H exceeds 32-bit indexing");
  return {T, T / L, H, NL};
}

HqHeadWeights head_tensors(const Op& c, const std::vector<Tensor>& w, const char* const (&names)[10], int64_t H, int64_t NL) {
  TORCH_CHECK(w.size() == 10, c.op, ": got ", w.size(), " head tensors, expected 10");
  const int64_t numel[10] = {H * H, H, NL * H, NL, H, 1, H, 1, 2 * H, 2};
  for (int i = 0; i < 10; ++i) c.holds(w[i], F32, names[i], numel[i]);
  return HqHeadWeights{ptr<float>(w[0]), ptr<float>(w[1]), ptr<float>(w[2]), ptr<float>(w[3]), ptr<float>(w[4]),
                       ptr<float>(w[5]), ptr<float>(w[6]), ptr<float>(w[7]), ptr<float>(w[8]), ptr<float>(w[9])};
}
const char* const kHeadWeightNames[10] = {"wp", "bp", "wc", "bc", "wrs", "brs", "wre", "bre", "wsp", "bsp"};
const char* const kHeadGradNames[10] = {"g_wp", "g_bp", "g_wc", "g_bc", "g_wrs", "g_brs", "g_wre", "g_bre", "g_wsp", "g_bsp"};

// returns logits [T,2], pooled [B,H], cls [B,NL], reg [B,2] (sigmoid outputs)
std::vector<Tensor> qa_heads_fwd(Tensor seq, int64_t L, std::vector<Tensor> w, double p, int64_t seed, int64_t opid) {
  const Op c("qa_heads_fwd", seq);
  const auto [T, B, H, NL] = heads_operands(c, seq, L, w);
  const HqHeadWeights hw = head_tensors(c, w, kHeadWeightNames, H, NL);
  c10::DeviceGuard g(c.dev);
  auto f = w[0].options();
  auto logits = at::empty({T, 2}, f);
  auto pooled = at::empty({B, H}, f);
  auto cls = at::empty({B, NL}, f);
  auto reg = at::empty({B, 2}, f);
  auto hpart = at::empty({(int64_t)hq_qa_heads_fwd_scratch((int)B, (int)H)}, f);
  hq_qa_heads_fwd(seq.data_ptr(), hw, ptr<float>(logits), ptr<float>(pooled), ptr<float>(cls), ptr<float>(reg),
                  ptr<float>(hpart), ticket(seq, 0), (int)B, (int)L, (int)H, (int)NL, (float)p, u32(seed), u32(opid),
                  cur_stream(), seq.scalar_type() == F32);
  return {logits, pooled, cls, reg};
}

// returns losses [6], dlog [T,2], dheads [B,16]
std::vector<Tensor> qa_loss(Tensor logits, Tensor cls, Tensor reg, Tensor t_start, Tensor t_end, Tensor t_rs, Tensor t_re,
                            Tensor t_cls, OptTensor lw, int64_t kind, int64_t ignore_cls, std::vector<double> weights,
                            double alpha, double gamma, double conf, double fill, OptTensor seg_len) {
  const Op c("qa_loss", logits);
  const auto [B, NL] = c.matrix(cls, "cls");
  const int64_t T = c.matrix(logits, "logits")[0];
  c.is(logits, F32, "logits", {T, 2});
  c.is(cls, F32, "cls", {B, NL});
  c.holds(reg, F32, "reg", 2 * B);
  c.holds(t_start, I64, "start_class", B);
  c.holds(t_end, I64, "end_class", B);
  c.holds(t_rs, F32, "start_reg", B);
  c.holds(t_re, F32, "end_reg", B);
  c.holds(t_cls, I64, "cls target", B);
  c.holds(lw, F32, "label_weights", NL);
  TORCH_CHECK(B > 0 && T % B == 0, "qa_loss: logits has ", T, " rows, expected a multiple of B = ", B);
  TORCH_CHECK(NL >= 1 && NL <= 8, "qa_loss: cls has ", NL, " classes, expected 1..8");
  TORCH_CHECK(weights.size() == 5 && kind >= 0 && kind <= 2, "loss config");
  int nseg = 1;
  if (has(seg_len)) {   // exact-objective merge: one segment per micro-batch
    c.dense(*seg_len, I32, "segment lengths");
    nseg = (int)seg_len->numel();
    TORCH_CHECK(nseg >= 1 && B % nseg == 0, "segments must split the batch into equal parts");
  }
  c10::DeviceGuard g(c.dev);
  auto f = logits.options();
  auto losses = at::empty({6}, f);
  auto dlog = at::empty({T, 2}, f);
  auto dheads = at::empty({B, 16}, f);
  auto part = at::empty({(int64_t)hq_qa_loss_partials((int)B), 4}, f);
  HqLossCfg cfg;
  cfg.kind = (int)kind;
  cfg.ignore_cls = (int)ignore_cls;
  for (int i = 0; i < 5; ++i) cfg.w[i] = (float)weights[i];
  cfg.alpha = (float)alpha; cfg.gamma = (float)gamma; cfg.conf = (float)conf; cfg.fill = (float)fill;
  hq_qa_loss(ptr<float>(logits), ptr<float>(cls), ptr<float>(reg), ptr<int64_t>(t_start), ptr<int64_t>(t_end),
             ptr<int64_t>(t_cls), ptr<float>(t_rs), ptr<float>(t_re), optr<float>(lw), ptr<float>(dlog), ptr<float>(dheads),
             ptr<float>(losses), ptr<float>(part), ticket(logits, 1), (int)B, (int)(T / B), (int)NL, cfg,
             optr<int>(seg_len), nseg, cur_stream());
  return {losses, dlog, dheads};
}

// writes the 10 head gradients (wp, bp, wc, bc, wrs, brs, wre, bre, wsp, bsp) (+)=; returns dseq (seq's dtype and shape)
Tensor qa_heads_bwd(Tensor seq, int64_t L, Tensor dlog, Tensor dheads, OptTensor gscale, Tensor pooled, Tensor reg,
                    std::vector<Tensor> w, std::vector<Tensor> grads, bool accumulate, double p, int64_t seed, int64_t opid) {
  const Op c("qa_heads_bwd", seq);
  const auto [T, B, H, NL] = heads_operands(c, seq, L, w);
  c.holds(dlog, F32, "dlog", 2 * T);
  c.holds(dheads, F32, "dheads", 16 * B);
  c.holds(gscale, F32, "gscale", 1);
  c.holds(pooled, F32, "pooled", B * H);
  c.holds(reg, F32, "reg", 2 * B);
  const HqHeadWeights hw = head_tensors(c, w, kHeadWeightNames, H, NL);
  const HqHeadWeights hg = head_tensors(c, grads, kHeadGradNames, H, NL);   // the gradients: the weights' contract
  HqHeadGrads gg{const_cast<float*>(hg.wp), const_cast<float*>(hg.bp), const_cast<float*>(hg.wc),
                 const_cast<float*>(hg.bc), const_cast<float*>(hg.wrs), const_cast<float*>(hg.brs),
                 const_cast<float*>(hg.wre), const_cast<float*>(hg.bre), const_cast<float*>(hg.wsp),
                 const_cast<float*>(hg.bsp)};
  c10::DeviceGuard g(c.dev);
  auto dseq = at::empty_like(seq);
  auto part = at::empty({(int64_t)hq_qa_heads_bwd_span_blocks((int)T), 2 * H + 2}, pooled.options());
  auto dpre = at::empty({B, H}, pooled.options());
  hq_qa_heads_bwd(seq.data_ptr(), ptr<float>(dlog), ptr<float>(dheads), optr<float>(gscale), ptr<float>(pooled),
                  ptr<float>(reg), hw, gg, dseq.data_ptr(), ptr<float>(part), (int)B, (int)L, (int)H, (int)NL,
                  accumulate, (float)p, u32(seed), u32(opid), cur_stream(), seq.scalar_type() == F32, ptr<float>(dpre));
  return dseq;
}

// ------------------------------------------------------------------ decode.hip: joint valid-span decoding
// start / end [B, L], cls [B, NL], start_reg / end_reg [B] are read in place through their strides (under no_grad the
// fused heads hand out stride-2 views of the logits and reg buffers); lo / hi int32 [B] contiguous.
HqDecodeIn decode_in(const Tensor& start, const Tensor& end, const Tensor& cls, const Tensor& start_reg,
                     const Tensor& end_reg, const Tensor& lo, const Tensor& hi) {
  const Op c("qa_decode", start);
  c.on(start, F32, "start"); c.on(end, F32, "end"); c.on(cls, F32, "cls");
  c.on(start_reg, F32, "start_reg"); c.on(end_reg, F32, "end_reg");
  TORCH_CHECK(start.dim() == 2 && end.dim() == 2 && cls.dim() == 2, "qa_decode: start / end [B, L], cls [B, NL]");
  const int64_t B = start.size(0), L = start.size(1), NL = cls.size(1);
  TORCH_CHECK(end.size(0) == B && end.size(1) == L && cls.size(0) == B, "qa_decode: start, end, cls disagree on B or L");
  TORCH_CHECK(L >= 1 && L <= kHqDecodeMaxL, "qa_decode supports 1 <= L <= ", kHqDecodeMaxL, ", got ", L);
  TORCH_CHECK(NL >= 1 && NL <= 8, "qa_decode supports 1..8 classes, got ", NL);
  TORCH_CHECK(start_reg.dim() == 1 && end_reg.dim() == 1 && start_reg.numel() == B && end_reg.numel() == B,
              "qa_decode: start_reg / end_reg must be [B]");
  c.holds(lo, I32, "lo", B);
  c.holds(hi, I32, "hi", B);
  HqDecodeIn in;
  in.start = ptr<float>(start); in.end = ptr<float>(end); in.cls = ptr<float>(cls);
  in.start_reg = ptr<float>(start_reg); in.end_reg = ptr<float>(end_reg);
  in.lo = ptr<int32_t>(lo); in.hi = ptr<int32_t>(hi);
  in.start_row = start.stride(0); in.start_elem = start.stride(1);
  in.end_row = end.stride(0); in.end_elem = end.stride(1);
  in.cls_row = cls.stride(0); in.cls_elem = cls.stride(1);
  in.start_reg_elem = start_reg.stride(0); in.end_reg_elem = end_reg.stride(0);
  return in;
}

// returns [B, 6] fp32 = (score, start, end, start_reg, end_reg, label)
Tensor qa_decode(Tensor start, Tensor end, Tensor cls, Tensor start_reg, Tensor end_reg, Tensor lo, Tensor hi, int64_t W) {
  const HqDecodeIn in = decode_in(start, end, cls, start_reg, end_reg, lo, hi);
  TORCH_CHECK(W >= 1, "qa_decode: max answer length must be >= 1, got ", W);
  const int64_t B = start.size(0), L = start.size(1);
  c10::DeviceGuard g(start.device());
  auto out = at::empty({B, 6}, start.options());
  if (B == 0) return out;
  hq_qa_decode(in, ptr<float>(out), (int)B, (int)L, (int)cls.size(1), (int)std::min<int64_t>(W, L), cur_stream());
  return out;
}

// tests: whether these inputs take the kernel's 8-byte interleaved loads (else scalar strided loads)
bool qa_decode_interleaved(Tensor start, Tensor end, Tensor cls, Tensor start_reg, Tensor end_reg, Tensor lo, Tensor hi) {
  return hq_qa_decode_interleaved(decode_in(start, end, cls, start_reg, end_reg, lo, hi));
}

}  // namespace

PYBIND11_MODULE(_hq_kernels, m) {
  m.doc() = "gfx950 HIP kernels + RCCL reducer for ml_recipe_distributed_pytorch_amd";
  // rowops
  m.def("set_dropout_seed", &set_dropout_seed);
  m.def("key_bias", &key_bias);
  m.def("gelu_fwd", &gelu_fwd);
  m.def("f32_gelu_fwd", &f32_gelu_fwd);
  m.def("gelu_bwd", &gelu_bwd);
  m.def("f32_gelu_bwd", &f32_gelu_bwd);
  m.def("bias_grad", &bias_grad);
  m.def("f32_colsum", &f32_colsum);
  m.def("colsum_into", &colsum_into);
  // norm
  m.def("ln_fwd", &ln_fwd, py::arg("a"), py::arg("resid"), py::arg("gamma"), py::arg("beta"), py::arg("eps"), py::arg("p"),
        py::arg("seed"), py::arg("opid"), py::arg("q8") = py::none(), py::arg("phase") = 0, py::arg("store_z") = true);
  m.def("f32_ln_fwd", &f32_ln_fwd);
  m.def("ln_bwd", &ln_bwd, py::arg("dy"), py::arg("dy2"), py::arg("z"), py::arg("gamma"), py::arg("mean"), py::arg("rstd"),
        py::arg("p"), py::arg("seed"), py::arg("opid"), py::arg("g_gamma"), py::arg("g_beta"), py::arg("g_bias"),
        py::arg("accumulate"), py::arg("q8") = py::none(), py::arg("phase") = 0, py::arg("write_da") = true,
        py::arg("beta") = py::none());
  m.def("f32_ln_bwd", &f32_ln_bwd, py::arg("dy"), py::arg("dy2"), py::arg("z"), py::arg("gamma"), py::arg("mean"),
        py::arg("rstd"), py::arg("p"), py::arg("seed"), py::arg("opid"), py::arg("g_gamma"), py::arg("g_beta"),
        py::arg("g_bias"), py::arg("accumulate"), py::arg("beta") = py::none());
  m.def("ln_guard", &ln_guard);
  // sort
  m.def("sort_ids", &sort_ids);
  // embedding
  m.def("embed_fwd", &embed_fwd);
  m.def("f32_embed_fwd", &f32_embed_fwd);
  m.def("embed_bwd", &embed_bwd, py::arg("dy"), py::arg("ids"), py::arg("pids"), py::arg("tids"), py::arg("ww"),
        py::arg("wp"), py::arg("wt"), py::arg("gamma"), py::arg("mean"), py::arg("rstd"), py::arg("p"), py::arg("seed"),
        py::arg("opid"), py::arg("g_word"), py::arg("g_pos"), py::arg("g_type"), py::arg("g_gamma"), py::arg("g_beta"),
        py::arg("accumulate"), py::arg("pad_word"), py::arg("pad_pos"), py::arg("seq_len") = 0,
        py::arg("deterministic") = false, py::arg("det_positions") = false);
  m.def("f32_embed_bwd", &f32_embed_bwd, py::arg("dy"), py::arg("ids"), py::arg("pids"), py::arg("tids"), py::arg("ww"),
        py::arg("wp"), py::arg("wt"), py::arg("gamma"), py::arg("mean"), py::arg("rstd"), py::arg("p"), py::arg("seed"),
        py::arg("opid"), py::arg("g_word"), py::arg("g_pos"), py::arg("g_type"), py::arg("g_gamma"), py::arg("g_beta"),
        py::arg("accumulate"), py::arg("pad_word"), py::arg("pad_pos"), py::arg("deterministic") = false);
  m.def("embed_run_chunk", []() { return kHqEmbRunChunk; });   // the unit of the sorted-run summation order
  // attention
  m.def("attn_set_force_slow", [](int64_t v) { hq_attn_set_force_slow((int)v); });
  m.def("attn_fwd", &attn_fwd, py::arg("qkv"), py::arg("key_bias"), py::arg("B"), py::arg("L"), py::arg("nh"),
        py::arg("p"), py::arg("seed"), py::arg("opid"), py::arg("scale"), py::arg("q8") = py::none(),
        py::arg("phase") = 0);
  m.def("f32_attn_fwd", &f32_attn_fwd);
  m.def("attn_bwd", &attn_bwd);
  m.def("attn_bwd_q8", &attn_bwd_q8, py::arg("dctx"), py::arg("qkv"), py::arg("ctx"), py::arg("lse"), py::arg("key_bias"),
        py::arg("mbits"), py::arg("B"), py::arg("L"), py::arg("nh"), py::arg("p"), py::arg("scale"),
        py::arg("deterministic"), py::arg("q8"), py::arg("phase"), py::arg("write_bf16") = true);
  m.def("f32_attn_bwd", &f32_attn_bwd);
  // optimizer
  m.def("grad_norm", &grad_norm);
  m.def("sq_norm_partials", &sq_norm_partials);
  m.def("fingerprint", &fingerprint);
  m.def("sq_norm_chunks", &sq_norm_chunks);
  m.def("clip_from_partials", &clip_from_partials);
  m.def("adamw", &adamw);
  m.def("adamod", &adamod);
  py::class_<LambPlan>(m, "LambPlan")
      .def_readonly("chunks", &LambPlan::chunks)
      .def_readonly("seg_first_chunk", &LambPlan::seg_first_chunk)
      .def_readonly("chunk_seg", &LambPlan::chunk_seg)
      .def_readonly("arena_numel", &LambPlan::arena_numel)
      .def_readonly("nchunks", &LambPlan::nchunks)
      .def_readonly("nseg", &LambPlan::nseg)
      .def_readonly("ngroups", &LambPlan::ngroups);
  m.def("lamb_plan", &lamb_plan, py::arg("master"), py::arg("chunks"), py::arg("seg_first_chunk"));
  m.def("lamb_moments", &lamb_moments);
  m.def("lamb_ratio", &lamb_ratio);
  m.def("lamb_apply", &lamb_apply);
  m.def("lamb_step", &lamb_step);
  m.def("cast_f32_bf16", &cast_f32_bf16);
  m.def("cast_bf16_f32", &cast_bf16_f32);
  // GEMMs
  m.def("gemm_nt", &gemm_nt, py::arg("A"), py::arg("B"), py::arg("epi"), py::arg("bias") = py::none(),
        py::arg("pre") = py::none(), py::arg("resid") = py::none(), py::arg("part") = py::none(),
        py::arg("out") = py::none(), py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("opid") = 0);
  m.def("gemm_nt_supported", &gemm_nt_supported);
  m.def("gemm_nt_part_rows", &gemm_nt_part_rows);
  m.def("gemm_nt_ws_floats", &gemm_nt_ws_floats);
  m.def("gemm_set_variant", [](int64_t v) { hq_gemm_set_variant((int)v); });
  m.def("gemm_set_store_policy", [](int64_t v) { hq_gemm_set_store_policy((int)v); });
  m.def("gemm_set_stagger", [](int64_t v) { hq_gemm_set_stagger((int)v); });
  m.def("gemm_set_sched", [](int64_t v) { hq_gemm_set_sched((int)v); });
  m.def("gemm_get_sched", []() { return (int64_t)hq_gemm_get_sched(); });
  m.def("gemm_f32", &gemm_f32, py::arg("A"), py::arg("B"), py::arg("C"), py::arg("M"), py::arg("N"), py::arg("K"),
        py::arg("sa"), py::arg("sb"), py::arg("sc"), py::arg("batch") = 1, py::arg("nb_in") = 1, py::arg("alpha") = 1.0,
        py::arg("bias") = py::none(), py::arg("R") = py::none(), py::arg("ldr") = 0,
        py::arg("mode") = "exact");
  m.def("gemm_tn", &gemm_tn, py::arg("dy"), py::arg("x"), py::arg("out"), py::arg("accumulate") = false,
        py::arg("splits") = 0, py::arg("bias_out") = py::none());
  m.def("gemm_tn_splits", &gemm_tn_splits);
  m.def("gemm_tn_set_variant", [](int64_t v) { hq_gemm_tn_set_variant((int)v); });
  m.def("gemm_tn8", &gemm_tn8);
  m.def("gemm_tn8_splits", &gemm_tn8_splits);
  m.def("gemm_fp8", &gemm_fp8, py::arg("A8"), py::arg("B8"), py::arg("epi"), py::arg("bias"), py::arg("sa"), py::arg("sb"),
        py::arg("pre") = py::none(), py::arg("out8") = py::none(), py::arg("state") = py::none(), py::arg("phase") = 0,
        py::arg("part") = py::none(), py::arg("resid") = py::none(), py::arg("write_out") = true);
  m.def("gemm_fp8_supported", &gemm_fp8_supported);
  m.def("gemm_fp8_set_variant", [](int64_t v) { hq_gemm_fp8_set_variant((int)v); });
  // fp8 quantisation
  m.def("fp8_quantize", &fp8_quantize);
  m.def("fp8_quant_delayed", &fp8_quant_delayed);
  m.def("fp8_quant_delayed_multi", &fp8_quant_delayed_multi);
  m.def("fp8_quant_multi_blocks", &fp8_quant_multi_blocks);
  m.def("fp8_fold_defer", [](bool on) { return hq_fp8_fold_defer(on ? 1 : 0); },
        "batch the delayed-scaling amax folds of the fp8 producers until fp8_fold_flush (False: flush, immediate folds)");
  m.def("fp8_fold_flush", []() { hq_fp8_fold_flush(); });
  m.def("fp8_fold_pending", []() { return hq_fp8_fold_pending(); });
  m.def("gelud_code", []() { return std::make_pair((double)kHqGdLo, (double)kHqGdStep); },
        "(lo, step) of the fp8 path's 8-bit gelu' code: g = lo + q·step");
  m.def("gelud_code_enc", []() { return std::make_pair((double)kHqGdInv, (double)kHqGdOff); },
        "(inv, off) of the encoder: q = round(fma(g, inv, off)), clamp 0..255 (fp32)");
  m.def("gelud_encode8", &gelud_encode8);
  // transpose
  m.def("transpose_tiles", &transpose_tiles);
  m.def("transpose_tiles8", &transpose_tiles8);
  // QA heads, decode
  m.def("span_fwd", &span_fwd);
  m.def("span_bwd", &span_bwd);
  m.def("qa_heads_fwd", &qa_heads_fwd);
  m.def("qa_loss", &qa_loss);
  m.def("qa_heads_bwd", &qa_heads_bwd);
  m.def("qa_decode", &qa_decode);
  m.def("qa_decode_interleaved", &qa_decode_interleaved);
  // RCCL reducer
  m.def("rccl_unique_id", []() { return py::bytes(hq_rccl_unique_id()); });
  py::class_<HqReducer>(m, "Reducer")
      .def(py::init([](int rank, int world, py::bytes uid, int device) {
             return new HqReducer(rank, world, std::string(uid), device);
           }))
      .def("allreduce_f32", &HqReducer::allreduce_f32, py::arg("ptr"), py::arg("count"), py::arg("stream"),
           py::arg("op") = 0, py::call_guard<py::gil_scoped_release>())
      .def("allreduce_bf16", &HqReducer::allreduce_bf16, py::call_guard<py::gil_scoped_release>())
      .def("broadcast", &HqReducer::broadcast, py::call_guard<py::gil_scoped_release>())
      .def("wait", &HqReducer::wait)
      .def("probe_f32", &HqReducer::probe_f32)
      .def("sq_norm_chunks", &HqReducer::sq_norm_chunks)
      .def("fence_from", &HqReducer::fence_from)
      .def("synchronize", &HqReducer::synchronize, py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("comm_stream", &HqReducer::comm_stream)
      .def_property_readonly("rank", &HqReducer::rank)
      .def_property_readonly("world", &HqReducer::world)
      .def_property_readonly("comm_count", &HqReducer::comm_count);
}
