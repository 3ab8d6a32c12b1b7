// Exact-fp32 GEMM on the gfx950 f32-input matrix cores (v_mfma_f32_32x32x2_f32) for --precision fp32
// (the reference's apex_level None / O0 mode: fp32 everywhere, /root/reference/modules/model/trainer/trainer.py:23-32,
// 128-133, 200-204).  The bf16 path never runs here; this kernel carries every GEMM-shaped FLOP of the fp32 mode:
// the encoder projections (forward, dgrad, weight gradient) and the attention's batched QKᵀ / PV products and their
// backward.
//
//   C[i, j] = alpha · Σ_k A(i, k) · B(j, k)  (+ bias[j])  (+ R[i, j])
//
// with strided operands A(i, k) = A[i·sa_i + k·sa_k] and B(j, k) = B[j·sb_j + k·sb_k], one of the two strides of each
// operand being 1 (A_K / B_K: the k stride is 1), so every layout the fp32 mode needs is a view, never a copy:
//   forward x·Wᵀ           A_K B_K      dgrad dy·W        A_K !B_K      weight grad dyᵀ·x    !A_K !B_K
// and the attention products through a two-level batch index z = outer·nb_in + inner (strides per operand).
//
// * 128 × 128 block tile, BK = 16, 256 threads = 4 waves as 2 × 2, each wave 64 × 64 = 2 × 2 MFMA 32×32 tiles
//   (64 accumulator VGPRs).  The MFMA operands are one f32 VGPR per lane: lane l reads A[i = l & 31][k = l >> 5]
//   and B[k = l >> 5][j = l & 31] — LDS holds both tiles k-major ([BK][128]), so the 32 lanes of a half-wave
//   read 32 consecutive words (conflict-free ds_read_b32).
// * Global → LDS by register staging (the k-contiguous operand is transposed in the write), double-buffered:
//   tile t+1's loads are issued before tile t's MFMAs, written to the other LDS buffer after them.
// * Numerics: each MFMA is a k-ordered f32 fma chain (exact f32 products, one rounding each, CDNA4 guide §3),
//   so the result matches an fp32 reference to ~1e-7·Σ|a·b|.
// * Split-K (ksplit > 1, unbatched): split s sums k-tiles [s·nk/ksplit, (s+1)·nk/ksplit) into fp32 slab ws[s];
//   gemm_f32_reduce_kernel folds the slabs in order (deterministic) and applies the epilogue.
#include "hq_common.h"
#include "hq_kernels.h"

namespace {

constexpr int TB = 128;      // block tile (rows = cols)
constexpr int BKF = 16;      // k per LDS stage
constexpr int LDS_ROW = TB;  // floats per k-row of a staged tile

struct F32Args {
  const float* A;
  const float* B;
  float* C;
  const float* bias;
  const float* R;
  float* ws;
  int M, N, K, ldc, ldr, nb_in, ksplit;
  long long sa_i, sa_k, sb_j, sb_k;
  long long ba_out, ba_in, bb_out, bb_in, bc_out, bc_in;
  float alpha;
};

// the [BKF][TB] k-major stage of one operand: rows r0.. of the operand (i or j), k-tile starting at k0
template <bool KC>
__device__ __forceinline__ void load_stage(const float* __restrict__ X, long long s_r, long long s_k, int rows, int K,
                                           int r0, int k0, int tid, float4 (&reg)[2]) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (KC) {                    // k contiguous: a float4 = 4 k of one row
      const int r = tid & 127, kq = (tid >> 7) + 2 * q;
      const int gr = r0 + r, gk = k0 + kq * 4;
      if (gr < rows && gk < K) v = *reinterpret_cast<const float4*>(X + gr * s_r + gk);
    } else {                               // row contiguous: a float4 = 4 rows of one k
      const int rq = tid & 31, kk = (tid >> 5) + 8 * q;
      const int gr = r0 + rq * 4, gk = k0 + kk;
      if (gr < rows && gk < K) v = *reinterpret_cast<const float4*>(X + gr + gk * s_k);
    }
    reg[q] = v;
  }
}

template <bool KC>
__device__ __forceinline__ void store_stage(float* __restrict__ lds, int tid, const float4 (&reg)[2]) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    if constexpr (KC) {
      const int r = tid & 127, kq = (tid >> 7) + 2 * q;
      lds[(kq * 4 + 0) * LDS_ROW + r] = reg[q].x;
      lds[(kq * 4 + 1) * LDS_ROW + r] = reg[q].y;
      lds[(kq * 4 + 2) * LDS_ROW + r] = reg[q].z;
      lds[(kq * 4 + 3) * LDS_ROW + r] = reg[q].w;
    } else {
      const int rq = tid & 31, kk = (tid >> 5) + 8 * q;
      *reinterpret_cast<float4*>(lds + kk * LDS_ROW + rq * 4) = reg[q];
    }
  }
}

template <bool A_K, bool B_K>
__global__ __launch_bounds__(256, 2) void gemm_f32_kernel(F32Args a) {
  __shared__ __attribute__((aligned(16))) float smem[2][2][BKF * LDS_ROW];   // [buf][A|B][k][row]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles_n = (a.N + TB - 1) / TB;
  const int tile = blockIdx.x;
  const int m0 = (tile / tiles_n) * TB, n0 = (tile % tiles_n) * TB;
  const int split = blockIdx.y;
  const int z = blockIdx.z, zo = z / a.nb_in, zi = z - zo * a.nb_in;
  const float* A = a.A + zo * a.ba_out + zi * a.ba_in;
  const float* B = a.B + zo * a.bb_out + zi * a.bb_in;
  const int nk = (a.K + BKF - 1) / BKF;
  const int kt0 = split * nk / a.ksplit, kt1 = (split + 1) * nk / a.ksplit;

  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float4 ra[2], rb[2];
  if (kt0 < kt1) {
    load_stage<A_K>(A, a.sa_i, a.sa_k, a.M, a.K, m0, kt0 * BKF, tid, ra);
    load_stage<B_K>(B, a.sb_j, a.sb_k, a.N, a.K, n0, kt0 * BKF, tid, rb);
    store_stage<A_K>(smem[0][0], tid, ra);
    store_stage<B_K>(smem[0][1], tid, rb);
  }
  __syncthreads();
  const int li = lane & 31, lk = lane >> 5;
  for (int kt = kt0; kt < kt1; ++kt) {
    const int buf = (kt - kt0) & 1;
    const bool more = kt + 1 < kt1;
    if (more) {
      load_stage<A_K>(A, a.sa_i, a.sa_k, a.M, a.K, m0, (kt + 1) * BKF, tid, ra);
      load_stage<B_K>(B, a.sb_j, a.sb_k, a.N, a.K, n0, (kt + 1) * BKF, tid, rb);
    }
    const float* As = smem[buf][0];
    const float* Bs = smem[buf][1];
#pragma unroll
    for (int ks = 0; ks < BKF; ks += 2) {
      float av[2], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) av[i] = As[(ks + lk) * LDS_ROW + wm * 64 + i * 32 + li];
#pragma unroll
      for (int j = 0; j < 2; ++j) bv[j] = Bs[(ks + lk) * LDS_ROW + wn * 64 + j * 32 + li];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      store_stage<A_K>(smem[buf ^ 1][0], tid, ra);
      store_stage<B_K>(smem[buf ^ 1][1], tid, rb);
    }
    __syncthreads();
  }

  // C/D map of the 32×32 MFMA: col = lane & 31, row = (r & 3) + 8·(r >> 2) + 4·(lane >> 5)
  const int col_l = lane & 31, row_h = 4 * (lane >> 5);
  HQ_DASSERT(split < a.ksplit && m0 < a.M && n0 < a.N);
  if (a.ksplit > 1) {
    HQ_DASSERT(a.ws != nullptr);
    float* slab = a.ws + (long long)split * a.M * a.N;   // slab `split` of the [ksplit][M][N] workspace
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int gj = n0 + wn * 64 + j * 32 + col_l;
        if (gj >= a.N) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int gi = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + row_h;
          if (gi < a.M) {
            HQ_DASSERT(gj < a.N);
            slab[(long long)gi * a.N + gj] = acc[i][j][r];
          }
        }
      }
    return;
  }
  float* C = a.C + zo * a.bc_out + zi * a.bc_in;
  const float* R = a.R ? a.R + zo * a.bc_out + zi * a.bc_in : nullptr;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int gj = n0 + wn * 64 + j * 32 + col_l;
      if (gj >= a.N) continue;
      const float bj = a.bias ? a.bias[gj] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gi = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + row_h;
        if (gi >= a.M) continue;
        float v = a.alpha * acc[i][j][r] + bj;
        HQ_DASSERT(gj < a.N && gj < a.ldc && (R == nullptr || gj < a.ldr));
        if (R) v += R[(long long)gi * a.ldr + gj];
        C[(long long)gi * a.ldc + gj] = v;
      }
    }
}

__global__ __launch_bounds__(256) void gemm_f32_reduce_kernel(const float* __restrict__ ws, int ksplit, float* __restrict__ C,
                                                              const float* __restrict__ bias, const float* __restrict__ R,
                                                              int M, int N, int ldc, int ldr, float alpha) {
  const long long n = (long long)M * N;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int k = 0; k < ksplit; ++k) s += ws[k * n + e];   // slab order: deterministic
    const int i = (int)(e / N), j = (int)(e - (long long)i * N);
    float v = alpha * s + (bias ? bias[j] : 0.f);
    if (R) v += R[(long long)i * ldr + j];
    C[(long long)i * ldc + j] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// bf16x3 split GEMM (HQ_F32_MATMUL=bf16x3 / --fp32_matmul bf16x3): the same contract on the bf16 matrix cores.
// Each fp32 operand element is written x ≈ hi + mid with hi = bf16_rne(x), mid = bf16_rne(x − float(hi)) (the
// subtraction is exact in fp32; |x − hi − mid| ≤ 2⁻¹⁶·|x|), and per 16-k chunk the one fp32 accumulator takes
// Amid·Bhi, then Ahi·Bmid, then Ahi·Bhi on v_mfma_f32_32x32x16_bf16: three bf16 MFMAs where the exact kernel
// spends eight f32 MFMAs of 1/16 the rate.  The dropped terms (mid·mid and the split remainders) bound the error
// at 3·2⁻¹⁶·Σ|a||b|.  An inf input gives hi = inf, mid = inf − inf = NaN; a NaN input gives NaN planes: either
// way every output the element feeds is non-finite.
//
// * 128 × 128 block tile, BK = 32, 4 waves as 2 × 2, each 2 × 2 MFMA tiles: per 16-k step a wave reads 8
//   fragments (A/B × hi/mid × 2 tiles) with ds_read_b128 and issues 12 MFMAs.  Two LDS stages and two register
//   stages: stage t's MFMAs run over the split + LDS write of stage t + 1 and the global loads of stage t + 2.
// * LDS: per operand a hi plane and a mid plane, row-major [128 rows][32 k] bf16 = 64-B rows of four 16-B chunks,
//   chunk c of row r stored at chunk c ^ ((r >> 2) & 3): a ds_read_b128 lane group ({0-3, 12-15, 20-27} …) then
//   covers the 16 slots of a 256-B bank row once.  64 KiB for the two stages, two workgroups per CU.
// * Both global layouts stage to this one image with 8-byte LDS writes.  The k-contiguous operand's float4 is
//   4 k of one row.  The row-contiguous operand's float4 is 4 rows of one k: a thread loads the same 4 rows at 4
//   consecutive k and transposes in registers (free), then writes its rows in an order that depends on bit 2 of
//   its row quad so that a 16-lane write group covers both 64-B halves of the 128-B write bank row.
constexpr int BKX = 32;                    // k per LDS stage
constexpr int X3_ROW_B = BKX * 2;          // bytes per row of a plane
constexpr int X3_PLANE_B = TB * X3_ROW_B;  // one plane of one operand stage

__device__ __forceinline__ int x3_off(int row, int chunk) { return row * X3_ROW_B + ((chunk ^ ((row >> 2) & 3)) << 4); }

// 4 consecutive k of one row -> 4 bf16 hi + 4 bf16 mid, stored at k quad kq (0..7) of that row
__device__ __forceinline__ void x3_split4(float x0, float x1, float x2, float x3, uint2& hi, uint2& mid) {
  hi = make_uint2(hq_pack2(x0, x1), hq_pack2(x2, x3));
  mid = make_uint2(hq_pack2(x0 - __uint_as_float(hi.x << 16), x1 - __uint_as_float(hi.x & 0xFFFF0000u)),
                   hq_pack2(x2 - __uint_as_float(hi.y << 16), x3 - __uint_as_float(hi.y & 0xFFFF0000u)));
}

__device__ __forceinline__ void x3_put(unsigned char* __restrict__ planes, int row, int kq, const uint2& hi,
                                       const uint2& mid) {
  const int o = x3_off(row, kq >> 1) + (kq & 1) * 8;
  HQ_DASSERT(row >= 0 && row < TB && kq >= 0 && kq < BKX / 4 && o + 8 <= X3_PLANE_B);
  *reinterpret_cast<uint2*>(planes + o) = hi;
  *reinterpret_cast<uint2*>(planes + X3_PLANE_B + o) = mid;
}

// Global -> registers, branch-free: a row or k index past the operand is clamped to its last valid quad, so every
// address lies inside the view the binding checked.  Rows past M / N then carry copies of valid rows and only feed
// outputs that are never stored; k past K is zeroed when the registers are split (x3_store_stage).
template <bool KC>
__device__ __forceinline__ void x3_load_stage(const float* __restrict__ X, long long s_r, long long s_k, int rows, int K,
                                              int r0, int k0, int tid, float4 (&reg)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if constexpr (KC) {                    // 8 lanes = 128 contiguous bytes of one row
      const int kq = tid & 7, r = (tid >> 3) + 32 * q;
      const int gr = min(r0 + r, rows - 1), gk = min(k0 + kq * 4, K - 4);
      HQ_DASSERT(gr >= 0 && gk >= 0 && (K & 3) == 0);
      reg[q] = *reinterpret_cast<const float4*>(X + gr * s_r + gk);
    } else {                               // 8 lanes = 32 contiguous rows of one k; q walks the thread's 4 k
      const int rq = (tid & 7) + 8 * (tid >> 6), kg = (tid >> 3) & 7;
      const int gr = min(r0 + rq * 4, rows - 4), gk = min(k0 + kg * 4 + q, K - 1);
      HQ_DASSERT(gr >= 0 && gk >= 0 && (rows & 3) == 0);
      reg[q] = *reinterpret_cast<const float4*>(X + gr + gk * s_k);
    }
  }
}

// registers of the stage at k0 -> hi / mid planes; k >= K becomes zero in both
template <bool KC>
__device__ __forceinline__ void x3_store_stage(unsigned char* __restrict__ planes, int tid, const float4 (&reg)[4],
                                               int k0, int K) {
  if constexpr (KC) {
    const int kq = tid & 7;
    const bool in = k0 + kq * 4 < K;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = (tid >> 3) + 32 * q;
      uint2 hi, mid;
      x3_split4(in ? reg[q].x : 0.f, in ? reg[q].y : 0.f, in ? reg[q].z : 0.f, in ? reg[q].w : 0.f, hi, mid);
      x3_put(planes, r, kq, hi, mid);
    }
  } else {
    const int rq = (tid & 7) + 8 * (tid >> 6), kg = (tid >> 3) & 7;
    const int kb = k0 + kg * 4;
    const bool i0 = kb < K, i1 = kb + 1 < K, i2 = kb + 2 < K, i3 = kb + 3 < K;
    uint2 h0, h1, h2, h3, m0, m1, m2, m3;
    x3_split4(i0 ? reg[0].x : 0.f, i1 ? reg[1].x : 0.f, i2 ? reg[2].x : 0.f, i3 ? reg[3].x : 0.f, h0, m0);
    x3_split4(i0 ? reg[0].y : 0.f, i1 ? reg[1].y : 0.f, i2 ? reg[2].y : 0.f, i3 ? reg[3].y : 0.f, h1, m1);
    x3_split4(i0 ? reg[0].z : 0.f, i1 ? reg[1].z : 0.f, i2 ? reg[2].z : 0.f, i3 ? reg[3].z : 0.f, h2, m2);
    x3_split4(i0 ? reg[0].w : 0.f, i1 ? reg[1].w : 0.f, i2 ? reg[2].w : 0.f, i3 ? reg[3].w : 0.f, h3, m3);
    // lanes with bit 2 of the row quad set write rows 1, 0, 3, 2: a 16-lane write group then covers both
    // 64-B halves of the 128-B write bank row
    const bool odd = (rq >> 2) & 1;
    const int e0 = odd ? 1 : 0, e1 = e0 ^ 1;
    x3_put(planes, rq * 4 + e0, kg, odd ? h1 : h0, odd ? m1 : m0);
    x3_put(planes, rq * 4 + e1, kg, odd ? h0 : h1, odd ? m0 : m1);
    x3_put(planes, rq * 4 + 2 + e0, kg, odd ? h3 : h2, odd ? m3 : m2);
    x3_put(planes, rq * 4 + 2 + e1, kg, odd ? h2 : h3, odd ? m2 : m3);
  }
}

// One k stage of a workgroup: the 2 × 12 MFMAs on LDS stage `cur`, with the split + LDS write of the NEXT stage's
// staged registers (xa, xb -> `nxt`) in the same basic block so that its VALU work issues under the MFMAs, and the
// global loads of the stage after that (-> ya, yb) issued first: two stages of load latency cover.
template <bool A_K, bool B_K>
__device__ __forceinline__ void x3_stage(const F32Args& a, const float* __restrict__ A, const float* __restrict__ B,
                                         int m0, int n0, int tid, int kt, int kt1,
                                         const unsigned char* __restrict__ cur, unsigned char* __restrict__ nxt,
                                         int a_row, int b_row, int lh, int sw,
                                         f32x16_t (&acc)[2][2], const float4 (&xa)[4], const float4 (&xb)[4],
                                         float4 (&ya)[4], float4 (&yb)[4]) {
  // unconditional (clamped past K): no branch in the stage, so loads, MFMAs and the split schedule as one block
  x3_load_stage<A_K>(A, a.sa_i, a.sa_k, a.M, a.K, m0, (kt + 2) * BKX, tid, ya);
  x3_load_stage<B_K>(B, a.sb_j, a.sb_k, a.N, a.K, n0, (kt + 2) * BKX, tid, yb);
  const unsigned char* As = cur;
  const unsigned char* Bs = cur + 2 * X3_PLANE_B;
#pragma unroll
  for (int ks = 0; ks < BKX / 16; ++ks) {
    const int co = ((2 * ks + lh) ^ sw) << 4;   // rows li + 32·i share (row >> 2) & 3
    bf16x8_t ah[2], am[2], bh[2], bm[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int o = a_row + i * 32 * X3_ROW_B + co;
      HQ_DASSERT(o + 16 <= X3_PLANE_B);
      ah[i] = *reinterpret_cast<const bf16x8_t*>(As + o);
      am[i] = *reinterpret_cast<const bf16x8_t*>(As + X3_PLANE_B + o);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int o = b_row + j * 32 * X3_ROW_B + co;
      HQ_DASSERT(o + 16 <= X3_PLANE_B);
      bh[j] = *reinterpret_cast<const bf16x8_t*>(Bs + o);
      bm[j] = *reinterpret_cast<const bf16x8_t*>(Bs + X3_PLANE_B + o);
    }
    // per accumulator and k chunk: the two small products first, then hi·hi — a fixed order
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bm[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
    // past the last stage this fills the buffer nobody reads again
    if (ks == 0) x3_store_stage<A_K>(nxt, tid, xa, (kt + 1) * BKX, a.K);
    else x3_store_stage<B_K>(nxt + 2 * X3_PLANE_B, tid, xb, (kt + 1) * BKX, a.K);
  }
}

template <bool A_K, bool B_K>
__global__ __launch_bounds__(256, 2) void gemm_f32x3_kernel(F32Args a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2][4 * X3_PLANE_B];   // [buf][A hi, A mid, B hi, B mid]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles_n = (a.N + TB - 1) / TB;
  // Workgroups go to the 8 XCDs round-robin by linear id.  Renumber so that one XCD's workgroups take consecutive
  // (tile, split) pairs: tiles of one A row panel, or all tiles of one k split, then share that XCD's L2.
  int lin = blockIdx.x + gridDim.x * blockIdx.y;
  const int nfull = (gridDim.x * gridDim.y) & ~7;
  if (lin < nfull) lin = (lin & 7) * (nfull >> 3) + (lin >> 3);
  const int tile = lin % gridDim.x, split = lin / gridDim.x;
  const int m0 = (tile / tiles_n) * TB, n0 = (tile % tiles_n) * TB;
  const int z = blockIdx.z, zo = z / a.nb_in, zi = z - zo * a.nb_in;
  const float* A = a.A + zo * a.ba_out + zi * a.ba_in;
  const float* B = a.B + zo * a.bb_out + zi * a.bb_in;
  const int nk = (a.K + BKX - 1) / BKX;
  const int kt0 = split * nk / a.ksplit, kt1 = (split + 1) * nk / a.ksplit;
  HQ_DASSERT((unsigned)tile < gridDim.x && split < a.ksplit && (int)gridDim.y == a.ksplit);

  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // register staging two stages deep: at stage t, (xa, xb) hold stage t + 1 and (ya, yb) receive stage t + 2
  float4 xa[4], xb[4], ya[4], yb[4];
  x3_load_stage<A_K>(A, a.sa_i, a.sa_k, a.M, a.K, m0, kt0 * BKX, tid, ya);
  x3_load_stage<B_K>(B, a.sb_j, a.sb_k, a.N, a.K, n0, kt0 * BKX, tid, yb);
  x3_load_stage<A_K>(A, a.sa_i, a.sa_k, a.M, a.K, m0, (kt0 + 1) * BKX, tid, xa);
  x3_load_stage<B_K>(B, a.sb_j, a.sb_k, a.N, a.K, n0, (kt0 + 1) * BKX, tid, xb);
  x3_store_stage<A_K>(smem[0], tid, ya, kt0 * BKX, a.K);
  x3_store_stage<B_K>(smem[0] + 2 * X3_PLANE_B, tid, yb, kt0 * BKX, a.K);
  __syncthreads();
  // fragment of the 32x32x16 MFMA: lane (li, lh) holds k = 8·lh … 8·lh + 7 of row li: chunk 2·ks + lh of k-step ks
  const int li = lane & 31, lh = lane >> 5, sw = (li >> 2) & 3;
  const int a_row = (wm * 64 + li) * X3_ROW_B, b_row = (wn * 64 + li) * X3_ROW_B;
  for (int kt = kt0; kt < kt1; kt += 2) {
    x3_stage<A_K, B_K>(a, A, B, m0, n0, tid, kt, kt1, smem[0], smem[1], a_row, b_row, lh, sw, acc, xa, xb, ya, yb);
    __syncthreads();
    if (kt + 1 >= kt1) break;
    x3_stage<A_K, B_K>(a, A, B, m0, n0, tid, kt + 1, kt1, smem[1], smem[0], a_row, b_row, lh, sw, acc, ya, yb, xa, xb);
    __syncthreads();
  }

  // C/D map and epilogue of the exact kernel
  const int col_l = lane & 31, row_h = 4 * (lane >> 5);
  HQ_DASSERT(split < a.ksplit && m0 < a.M && n0 < a.N);
  if (a.ksplit > 1) {
    HQ_DASSERT(a.ws != nullptr);
    float* slab = a.ws + (long long)split * a.M * a.N;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int gj = n0 + wn * 64 + j * 32 + col_l;
        if (gj >= a.N) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int gi = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + row_h;
          if (gi < a.M) {
            HQ_DASSERT(gj < a.N);
            slab[(long long)gi * a.N + gj] = acc[i][j][r];
          }
        }
      }
    return;
  }
  float* C = a.C + zo * a.bc_out + zi * a.bc_in;
  const float* R = a.R ? a.R + zo * a.bc_out + zi * a.bc_in : nullptr;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int gj = n0 + wn * 64 + j * 32 + col_l;
      if (gj >= a.N) continue;
      const float bj = a.bias ? a.bias[gj] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gi = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + row_h;
        if (gi >= a.M) continue;
        float v = a.alpha * acc[i][j][r] + bj;
        HQ_DASSERT(gj < a.N && gj < a.ldc && (R == nullptr || gj < a.ldr));
        if (R) v += R[(long long)gi * a.ldr + gj];
        C[(long long)gi * a.ldc + gj] = v;
      }
    }
}

}  // namespace

int hq_gemm_f32_splits(int M, int N, int K, int batch) {
  // enough workgroups to fill 256 CUs at 2 per CU when the output alone cannot (the weight gradients:
  // dW[768, 768] is 36 tiles over K = 98304 tokens); each split keeps >= 64 k-tiles
  const int tiles = ((M + TB - 1) / TB) * ((N + TB - 1) / TB) * batch;
  if (batch > 1 || tiles >= 256) return 1;
  const int nk = (K + BKF - 1) / BKF;
  int s = (512 + tiles - 1) / tiles;
  s = std::min(s, std::max(1, nk / 64));
  return std::max(1, std::min(s, 64));
}

void hq_gemm_f32(const float* A, const float* B, float* C, const float* bias, const float* R, float* ws, int M, int N,
                 int K, long long sa_i, long long sa_k, long long sb_j, long long sb_k, int ldc, int ldr, int batch,
                 int nb_in, long long ba_out, long long ba_in, long long bb_out, long long bb_in, long long bc_out,
                 long long bc_in, float alpha, int ksplit, hipStream_t s) {
  F32Args a{A, B, C, bias, R, ws, M, N, K, ldc, ldr, nb_in, ksplit, sa_i, sa_k, sb_j, sb_k,
            ba_out, ba_in, bb_out, bb_in, bc_out, bc_in, alpha};
  const int tiles = ((M + TB - 1) / TB) * ((N + TB - 1) / TB);
  dim3 grid(tiles, ksplit, batch);
  const bool ak = sa_k == 1, bk = sb_k == 1;
  if (ak && bk) gemm_f32_kernel<true, true><<<grid, 256, 0, s>>>(a);
  else if (ak) gemm_f32_kernel<true, false><<<grid, 256, 0, s>>>(a);
  else if (bk) gemm_f32_kernel<false, true><<<grid, 256, 0, s>>>(a);
  else gemm_f32_kernel<false, false><<<grid, 256, 0, s>>>(a);
  if (ksplit > 1) {
    const long long n = (long long)M * N;
    const int blocks = (int)std::min<long long>((n + 255) / 256, 2048);
    gemm_f32_reduce_kernel<<<blocks, 256, 0, s>>>(ws, ksplit, C, bias, R, M, N, ldc, ldr, alpha);
  }
}

void hq_gemm_f32x3(const float* A, const float* B, float* C, const float* bias, const float* R, float* ws, int M, int N,
                   int K, long long sa_i, long long sa_k, long long sb_j, long long sb_k, int ldc, int ldr, int batch,
                   int nb_in, long long ba_out, long long ba_in, long long bb_out, long long bb_in, long long bc_out,
                   long long bc_in, float alpha, int ksplit, hipStream_t s) {
  F32Args a{A, B, C, bias, R, ws, M, N, K, ldc, ldr, nb_in, ksplit, sa_i, sa_k, sb_j, sb_k,
            ba_out, ba_in, bb_out, bb_in, bc_out, bc_in, alpha};
  const int tiles = ((M + TB - 1) / TB) * ((N + TB - 1) / TB);
  dim3 grid(tiles, ksplit, batch);
  const bool ak = sa_k == 1, bk = sb_k == 1;
  if (ak && bk) gemm_f32x3_kernel<true, true><<<grid, 256, 0, s>>>(a);
  else if (ak) gemm_f32x3_kernel<true, false><<<grid, 256, 0, s>>>(a);
  else if (bk) gemm_f32x3_kernel<false, true><<<grid, 256, 0, s>>>(a);
  else gemm_f32x3_kernel<false, false><<<grid, 256, 0, s>>>(a);
  if (ksplit > 1) {
    const long long n = (long long)M * N;
    const int blocks = (int)std::min<long long>((n + 255) / 256, 2048);
    gemm_f32_reduce_kernel<<<blocks, 256, 0, s>>>(ws, ksplit, C, bias, R, M, N, ldc, ldr, alpha);
  }
}
