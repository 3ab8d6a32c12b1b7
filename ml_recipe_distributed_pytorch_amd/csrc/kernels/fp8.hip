// OCP fp8 (e4m3fn) quantisation for --precision fp8 (the GEMMs are gemm_fp8.hip's own block-scaled MFMA kernels).
// No host synchronisation anywhere.
// Current (just-in-time) per-tensor scaling, the standalone form:
//   hq_amax_bf16 : amax = max |x|                          (grid-wide max via float-as-uint atomics)
//   hq_fp8_quant : y = sat(x · 448 / amax) → e4m3fn,  scale = amax / 448 (the dequant factor the fp8 GEMM
//                  multiplies back in), both read from / written to device memory.
// Delayed scaling, the training step's form (second half of the file): the quantisers, the per-wave amax-partials
// arena every fp8 producer writes (LN, attention, the GEMM epilogues) and the fold kernels that reduce it into the
// 4-float state, immediate or deferred and batched.
// v_cvt_pk_fp8_f32 converts two f32 to OCP e4m3 on gfx950; inputs are clamped to ±448 first so an
// out-of-range value saturates instead of becoming NaN (e4m3fn has no infinity).
#include <algorithm>
#include <cstdio>
#include <vector>

#include "hq_common.h"
#include "hq_kernels.h"

namespace {

__global__ __launch_bounds__(256) void amax_kernel(const uint16_t* __restrict__ x, size_t n8, unsigned* __restrict__ amax) {
  float m = 0.f;
  for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
    float f[8];
    hq_unpack8(reinterpret_cast<const uint4*>(x)[i], f);
#pragma unroll
    for (int k = 0; k < 8; ++k) m = fmaxf(m, fabsf(f[k]));
  }
  m = hq_wave_max(m);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    atomicMax(amax, __float_as_uint(m));  // non-negative floats order like their bit patterns
  }
}

__global__ __launch_bounds__(256) void fp8_quant_kernel(const uint16_t* __restrict__ x, uint2* __restrict__ y, size_t n8,
                                                        const unsigned* __restrict__ amax, float* __restrict__ scale) {
  const float a = fmaxf(__uint_as_float(*amax), 1e-12f);
  const float inv = kHqFp8Max / a;
  if (blockIdx.x == 0 && threadIdx.x == 0) *scale = a / kHqFp8Max;
  for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
    float f[8];
    hq_unpack8(reinterpret_cast<const uint4*>(x)[i], f);
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = fminf(fmaxf(f[k] * inv, -kHqFp8Max), kHqFp8Max);
    uint32_t lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
    uint32_t hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
    y[i] = make_uint2(lo, hi);
  }
}

int grid_for(size_t n8) { return (int)std::min<size_t>((n8 + 255) / 256, 256 * 8); }

// bf16 gelu' -> the 8-bit code with the very encoder the fp8 FFN1 epilogue uses (hq_gd_encode8): for a bf16 gelu'
// that must meet the fp8 FFN2 dgrad (ops.gelud_encode)
__global__ __launch_bounds__(256) void gelud_encode8_kernel(const uint4* __restrict__ g, uint2* __restrict__ q, size_t n8) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
    float f[8];
    hq_unpack8(g[i], f);
    q[i] = hq_gd_encode8(f);
  }
}

}  // namespace

void hq_gelud_encode8(const uint16_t* g, uint8_t* q, size_t n, hipStream_t s) {
  const size_t n8 = n / 8;
  const int grid = std::max(1, (int)std::min<size_t>((n8 + 255) / 256, 4096));
  hipLaunchKernelGGL(gelud_encode8_kernel, dim3(grid), dim3(256), 0, s, reinterpret_cast<const uint4*>(g),
                     reinterpret_cast<uint2*>(q), n8);
}

void hq_amax_bf16(const uint16_t* x, size_t n, unsigned* amax, hipStream_t s) {
  hq_zero_f32(reinterpret_cast<float*>(amax), 1, s);   // own kernel: no runtime memset node under graph capture
  const size_t n8 = n / 8;
  if (n8) hipLaunchKernelGGL(amax_kernel, dim3(grid_for(n8)), dim3(256), 0, s, x, n8, amax);
}

void hq_fp8_quant(const uint16_t* x, uint8_t* y, size_t n, const unsigned* amax, float* scale, hipStream_t s) {
  const size_t n8 = n / 8;
  hipLaunchKernelGGL(fp8_quant_kernel, dim3(grid_for(n8 ? n8 : 1)), dim3(256), 0, s, x, reinterpret_cast<uint2*>(y), n8,
                     amax, scale);
}

namespace {

// ------------------------------------------------------------------ delayed-scaling quantiser
// y = e4m3(x / s), s = 2·amax_prev/448 from state slot (phase+2)%3 (unit when unset); this call's amax
// into slot `phase`, slot (phase+1)%3 cleared, s stored in state[3].  One read of x instead of the
// current-scaling path's two.
__global__ __launch_bounds__(256) void quant_delayed_kernel(const uint16_t* __restrict__ x, uint2* __restrict__ y, size_t n8,
                                                            const float* __restrict__ q8, float* __restrict__ part,
                                                            int phase) {
  hq_fp8_publish_scale(q8, phase);
  const float s = hq_fp8_delayed_scale(q8, phase);   // first step: unit scale
  const float inv = 1.f / s;
  float m = 0.f;
  for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
    float f[8];
    hq_unpack8(reinterpret_cast<const uint4*>(x)[i], f);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      m = fmaxf(m, fabsf(f[k]));
      f[k] = fminf(fmaxf(f[k] * inv, -kHqFp8Max), kHqFp8Max);
    }
    uint32_t lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
    uint32_t hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
    y[i] = make_uint2(lo, hi);
  }
  m = hq_wave_max(m);
  if ((threadIdx.x & 63) == 0) part[blockIdx.x * 4 + (threadIdx.x >> 6)] = m;
}

// Every weight of the model in ONE launch (ParamStore.view_fp8 after each optimizer step): segment g is
// x[xo, xo + 8·n8) -> y[yo, …) under its own state states[g]; a block handles kQmBlk8 8-element groups
// of one segment (segment g owns blocks blk[g] … blk[g+1]-1).  Same math as quant_delayed_kernel; the
// per-block amax only reaches the atomic when it beats the slot's current value (monotonic, so a stale
// read costs at most a redundant atomic) — 48 launches of ~13 µs each become one bandwidth-bound pass.
constexpr int kQmBlk8 = 256 * 8;
__global__ __launch_bounds__(256) void quant_delayed_multi_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ y,
                                                                  const long long* __restrict__ seg, int nseg,
                                                                  const float* __restrict__ states,
                                                                  float* __restrict__ part, int phase) {
  int g = 0;
  while (g + 1 < nseg && (long long)blockIdx.x >= seg[4 * (g + 1) + 3]) ++g;   // uniform scan, nseg <= ~100
  const long long xo = seg[4 * g], yo = seg[4 * g + 1], n8 = seg[4 * g + 2], b0 = seg[4 * g + 3];
  const float* q8 = states + 4 * g;
  const float s = hq_fp8_delayed_scale(q8, phase);   // first step: unit scale
  const float inv = 1.f / s;
  const uint4* xs = reinterpret_cast<const uint4*>(x + xo);
  uint2* ys = reinterpret_cast<uint2*>(y + yo);
  const long long i0 = ((long long)blockIdx.x - b0) * kQmBlk8;
  const long long i1 = i0 + kQmBlk8 < n8 ? i0 + kQmBlk8 : n8;
  float m = 0.f;
  for (long long i = i0 + threadIdx.x; i < i1; i += 256) {
    float f[8];
    hq_unpack8(xs[i], f);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      m = fmaxf(m, fabsf(f[k]));
      f[k] = fminf(fmaxf(f[k] * inv, -kHqFp8Max), kHqFp8Max);
    }
    uint32_t lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
    uint32_t hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
    ys[i] = make_uint2(lo, hi);
  }
  m = hq_wave_max(m);
  if ((threadIdx.x & 63) == 0) part[blockIdx.x * 4 + (threadIdx.x >> 6)] = m;
}

// ------------------------------------------------------------------ amax fold
// The fp8 producers (LN forward, attention ctx store, FFN1 epilogue, the quantisers) write one amax per
// wave into a scratch array instead of atomics on the state word: tens of thousands of same-address
// atomics serialise in one L2 channel (measured: 36.9 K per-wave atomics turned a 236 µs attention
// forward into 967 µs).  This single-block kernel then folds the partials into slot `phase`, clears slot
// (phase+1)%3 and stores the scale the producer used in state[3] — segment g of a multi-segment call
// (blockIdx.x = g) folds partials [4·blk[g], 4·blk[g+1]).
__device__ __forceinline__ void amax_fold_segment(const float* __restrict__ part, long long i0, long long i1,
                                                  float* __restrict__ q8, int phase, float fmax) {
  // partial counts are multiples of 4 (4 or 8 waves per producer block): float4 loads, 4 in flight
  const float4* p4 = reinterpret_cast<const float4*>(part);
  const long long j0 = i0 >> 2, j1 = i1 >> 2;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = a;
  long long j = j0 + threadIdx.x;
  for (; j + 3 * 1024 < j1; j += 4 * 1024) {
    const float4 v0 = p4[j], v1 = p4[j + 1024], v2 = p4[j + 2048], v3 = p4[j + 3072];
    a.x = fmaxf(fmaxf(a.x, v0.x), v1.x); a.y = fmaxf(fmaxf(a.y, v0.y), v1.y);
    a.z = fmaxf(fmaxf(a.z, v0.z), v1.z); a.w = fmaxf(fmaxf(a.w, v0.w), v1.w);
    c.x = fmaxf(fmaxf(c.x, v2.x), v3.x); c.y = fmaxf(fmaxf(c.y, v2.y), v3.y);
    c.z = fmaxf(fmaxf(c.z, v2.z), v3.z); c.w = fmaxf(fmaxf(c.w, v2.w), v3.w);
  }
  for (; j < j1; j += 1024) {
    const float4 v = p4[j];
    a.x = fmaxf(a.x, v.x); a.y = fmaxf(a.y, v.y); a.z = fmaxf(a.z, v.z); a.w = fmaxf(a.w, v.w);
  }
  float m = fmaxf(fmaxf(fmaxf(a.x, a.y), fmaxf(a.z, a.w)), fmaxf(fmaxf(c.x, c.y), fmaxf(c.z, c.w)));
  m = hq_wave_max(m);
  __shared__ float red[16];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < 16; ++w) m = fmaxf(m, red[w]);   // m = red[0] here (thread 0's wave)
    unsigned* st = reinterpret_cast<unsigned*>(q8);
    const float s = hq_fp8_delayed_scale(q8, phase, fmax);   // 448 (e4m3) or 57344 (e5m2 gradients)
    st[phase] = __float_as_uint(fmaxf(__uint_as_float(st[phase]), m));
    st[(phase + 1) % 3] = 0u;   // cleared for the step after next's accumulation
    q8[3] = s;                  // dequant scale of this step's e4m3 output
  }
}

__global__ __launch_bounds__(1024) void amax_fold_kernel(const float* __restrict__ part, const long long* __restrict__ seg,
                                                         int nseg, long long nblk, int n, float* __restrict__ states,
                                                         int phase, float fmax) {
  const int g = blockIdx.x;
  long long i0 = 0, i1 = n;
  if (seg != nullptr) {
    i0 = 4 * seg[4 * g + 3];
    i1 = 4 * (g + 1 < nseg ? seg[4 * (g + 1) + 3] : nblk);
  }
  amax_fold_segment(part, i0, i1, states + 4 * g, phase, fmax);
}

// Deferred folds (hq_fp8_fold_defer): up to kFoldBatch sites' folds in ONE launch, block g = site g — the ~97
// per-site single-block launches of an fp8 training step (~5 µs each, mostly launch and drain) become a handful.
struct FoldSeg {
  const float* part;
  float* q8;
  int n, phase;
  float fmax;
  int pad;
};
constexpr int kFoldBatch = 32;
struct FoldBatch {
  FoldSeg s[kFoldBatch];
};
__global__ __launch_bounds__(1024) void amax_fold_batch_kernel(FoldBatch b) {
  const FoldSeg& g = b.s[blockIdx.x];
  amax_fold_segment(g.part, 0, g.n, g.q8, g.phase, g.fmax);
}

// Per-device deferral state: partial slots come from one arena, bump-allocated and reset when the pending folds are
// launched, so every pending site keeps its own partials until its fold has read them.
struct FoldDefer {
  bool on = false;
  float* arena = nullptr;
  size_t cap = 0, used = 0;
  hipStream_t stream = nullptr;
  std::vector<FoldSeg> pending;
};
constexpr size_t kFoldArena = size_t(8) << 20;   // floats (32 MiB): a BERT-large step's partials with room to spare
FoldDefer& fold_defer() {
  static std::vector<FoldDefer> st;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if ((int)st.size() <= dev) st.resize(dev + 1);
  return st[dev];
}

void fold_flush(FoldDefer& d) {
  for (size_t i = 0; i < d.pending.size(); i += kFoldBatch) {
    FoldBatch b{};
    const int n = (int)std::min<size_t>(kFoldBatch, d.pending.size() - i);
    for (int j = 0; j < n; ++j) b.s[j] = d.pending[i + j];
    hipLaunchKernelGGL(amax_fold_batch_kernel, dim3(n), dim3(1024), 0, d.stream, b);
  }
  d.pending.clear();
  d.used = 0;   // stream order: the folds above read the arena before any later producer on d.stream writes it
}

}  // namespace

long long hq_fp8_quant_multi_blocks(long long n8) { return (n8 + kQmBlk8 - 1) / kQmBlk8; }

void hq_fp8_quant_delayed_multi(const uint16_t* x, uint8_t* y, const long long* seg, int nseg, long long blocks,
                                float* states, int phase, hipStream_t s) {
  if (blocks <= 0 || nseg <= 0) return;
  float* part = hq_fp8_amax_parts((size_t)blocks * 4);
  hipLaunchKernelGGL(quant_delayed_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, y, seg, nseg, states, part,
                     phase);
  hipLaunchKernelGGL(amax_fold_kernel, dim3(nseg), dim3(1024), 0, s, part, seg, nseg, blocks, 0, states, phase, kHqFp8Max);
}

float* hq_fp8_amax_parts(size_t n, const float* q8, hipStream_t s) {
  FoldDefer& d = fold_defer();
  if (d.on && q8 != nullptr) {
    // a site whose previous production still has a pending fold (its next scale reads that fold's slot), or a
    // producer on another stream (unordered against the pending folds' partials): launch the pending folds first
    bool flush = !d.pending.empty() && s != d.stream;
    for (const FoldSeg& g : d.pending) flush = flush || g.q8 == q8;
    const size_t n4 = (n + 3) & ~size_t(3);
    if (flush || d.used + n4 > d.cap) fold_flush(d);
    if (n4 <= d.cap) {
      float* p = d.arena + d.used;
      d.used += n4;
      d.stream = s;
      return p;
    }
  }
  // immediate mode: per-device scratch, grown on demand and never freed while kernels may still read it (the old
  // block is kept: a grow happens a handful of times per process).  Producers and their fold share one stream.
  static std::vector<std::pair<float*, size_t>> bufs;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if ((int)bufs.size() <= dev) bufs.resize(dev + 1, {nullptr, 0});
  auto& b = bufs[dev];
  if (b.second < n) {
    const size_t cap = std::max<size_t>(n, 1 << 18);
    float* p = nullptr;
    if (hipMalloc(&p, cap * sizeof(float)) != hipSuccess) { fprintf(stderr, "hq_fp8_amax_parts: hipMalloc failed\n"); abort(); }
    b = {p, cap};
  }
  return b.first;
}

void hq_fp8_amax_fold(const float* part, int n, float* q8, int phase, hipStream_t s, float fmax) {
  if (n % 4 != 0) { fprintf(stderr, "hq_fp8_amax_fold: %d partials (must be a multiple of 4)\n", n); abort(); }
  FoldDefer& d = fold_defer();
  if (d.on && part >= d.arena && part < d.arena + d.cap && s == d.stream) {
    d.pending.push_back(FoldSeg{part, q8, n, phase, fmax, 0});
    return;
  }
  hipLaunchKernelGGL(amax_fold_kernel, dim3(1), dim3(1024), 0, s, part, nullptr, 1, 0LL, n, q8, phase, fmax);
}

void hq_fp8_fold_flush() { fold_flush(fold_defer()); }

int hq_fp8_fold_defer(int on) {
  FoldDefer& d = fold_defer();
  if (!on) {
    fold_flush(d);
    d.on = false;
    return 0;
  }
  if (d.arena == nullptr) {   // allocated once, outside any graph capture (the first deferred step is eager)
    if (hipMalloc(&d.arena, kFoldArena * sizeof(float)) != hipSuccess) {
      fprintf(stderr, "hq_fp8_fold_defer: hipMalloc failed\n");
      abort();
    }
    d.cap = kFoldArena;
  }
  d.on = true;
  return 0;
}

int hq_fp8_fold_pending() { return (int)fold_defer().pending.size(); }

void hq_fp8_quant_delayed(const uint16_t* x, uint8_t* y, size_t n, float* q8, int phase, hipStream_t s) {
  const size_t n8 = n / 8;
  const int grid = std::max(1, (int)std::min<size_t>((n8 + 255) / 256, 256 * 8));
  float* part = hq_fp8_amax_parts((size_t)grid * 4, q8, s);
  hipLaunchKernelGGL(quant_delayed_kernel, dim3(grid), dim3(256), 0, s, x, reinterpret_cast<uint2*>(y), n8, q8, part,
                     phase);
  hq_fp8_amax_fold(part, grid * 4, q8, phase, s);
}
