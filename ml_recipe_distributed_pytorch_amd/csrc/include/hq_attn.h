// Private to the bf16 attention kernels (attention_fwd.hip, attention_bwd.hip) and tools/attn_lab: flash attention
// for BERT (head_dim 64, L <= 512, additive key mask, fused dropout) on gfx950.
//
// Input is the packed QKV GEMM output [T, 3H] (token-major; head h of Q/K/V at column {0,H,2H} + 64h), so no
// head-split transpose is ever materialised; ctx is written straight in [T, H] and the backward writes dQ/dK/dV
// straight into packed dQKV [T, 3H].
//
// Structure ("ring"): a workgroup is RW waves × 32 rows (queries for the forward and dQ, keys for dK/dV) of one
// head, and the other side of the head streams past it in 32-row tiles through a small LDS ring, so several
// workgroups share a CU and one's loads overlap the others' MFMAs.  (Keeping a whole head's K and V resident,
// 96 KB at L = 384, left one workgroup per CU whose load prologue and store epilogue overlapped nothing: 151 of
// 285 µs at B = 256, profiles/s3_prof/attn_lab.txt.)  blockIdx is remapped so the blocks of one head are
// consecutive on ONE XCD (they run together and read K/V through the same L2).
//
// MFMA: v_mfma_f32_32x32x16_bf16 (32x32 tile, K=16, wave64).  Orientation keeps every softmax statistic lane-local:
//   fwd : Sᵀ = K·Qᵀ (query on the lane); Oᵀ += Vᵀ·Pᵀ with Pᵀ fed from the accumulator registers as the B operand
//         (cdna_hip_programming.md §3) and Vᵀ via ds_read_b64_tr_b16 (T10).
//   dQ  : Sᵀ, dPᵀ = V·dOᵀ (query on the lane); dQᵀ += Kᵀ·dSᵀ.  Also computes δ = rowsum(dO·O).
//   dKdV: S = Q·Kᵀ, dP = dO·Vᵀ (key on the lane); dVᵀ += dOᵀ·Pd, dKᵀ += Qᵀ·dS.
// The key-mask bias (and the forward's row max, the backward's −LSE) ride in a 5th score MFMA on augmented operands,
// so the scores leave the MFMA ready for exp2.
// Dropout: the forward draws keep bits from the counter hash (hq_common.h, element index ((b·nh+h)·L+q)·L+k,
// bit-identical to ops/rng.py) and stores them as one 16-bit word per lane per 32×32 subtile (14 MB per BERT-base
// layer at B=64); the backward kernels read the bits instead of re-hashing.
#pragma once
#include <type_traits>

#include "hq_common.h"
#include "hq_kernels.h"

namespace {

constexpr int D = 64;  // head dim
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr int RW = 4;                    // waves per workgroup
constexpr int RQ = RW * 32;              // rows per workgroup
constexpr int RTILE = 32 * D * 2;        // bytes of one 32-row tile of K, V, Q or dO

typedef __attribute__((address_space(3))) bf16x4_t lds_bf16x4;
typedef __attribute__((address_space(3))) void al_void;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef uint16_t u16x2_t __attribute__((ext_vector_type(2)));
// Packed-f32 pair (v_pk_add/mul/fma_f32 on gfx950: two lanes' worth of f32 work per VALU issue).
typedef float f2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f32x16_t mfma32(const bf16x8_t& a, const bf16x8_t& b, const f32x16_t& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// LDS images are [rows][64] bf16 (128-B rows) with the 16-B chunk index XOR-swizzled by
//   f(row) = ((row>>1)&1)<<2 | ((row>>3)&3)
// found by exhaustive search (tools/lds_swizzle_search.py) to make BOTH access patterns bank-conflict
// free: ds_read_b128 row reads (16 rows of a lane group, one chunk) and ds_read_b64_tr_b16 reads
// (4 rows × 64 B per 32-lane half).  Unswizzled the row reads are 8-way conflicted (T2).
__device__ __forceinline__ int swz(int row) { return (((row >> 1) & 1) << 2) | ((row >> 3) & 3); }
__device__ __forceinline__ int lds_off(int row, int col) {  // element offset of (row, col)
  return row * D + ((((col >> 3) ^ swz(row)) << 3) | (col & 7));
}

// swz(row) only depends on row bits 1..4, so every offset inside a 32-row subtile is a lane constant:
// precompute them once (12 VGPRs) instead of re-deriving the XOR per access in VALU-bound loops.
struct LdsOffsets {
  int row[4];        // ds_read_b128 row reads: row (lane&31), chunk 16s + 8hh
  int tr[2][2][2];   // ds_read_b64_tr_b16: [s][dblk][lo/hi]
  __device__ __forceinline__ void init(int lane) {
    const int hh = lane >> 5;
#pragma unroll
    for (int s = 0; s < 4; ++s) row[s] = lds_off(lane & 31, 16 * s + 8 * hh);
    const int g = lane >> 4, i = lane & 15;
    const int th = g >> 1, dsub = g & 1;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const int r = 16 * s + 4 * th + (i >> 2);
        const int c = d * 32 + 16 * dsub + 4 * (i & 3);
        tr[s][d][0] = lds_off(r, c);
        tr[s][d][1] = lds_off(r + 8, c);
      }
  }
};

__device__ __forceinline__ bf16x8_t row8(const uint16_t* tile, int row0, const LdsOffsets& o, int s) {
  return *reinterpret_cast<const bf16x8_t*>(tile + row0 * D + o.row[s]);
}

// A operand "Xᵀ" of a 32x32x16 MFMA from a row-major [rows][64] LDS image: lane supplies X[row(s,hh,j)][d],
// d = dblk*32 + (lane&31), row = row0 + 16s + 4hh + (j&3) + 8(j>>2) (the k order of an accumulator-fed B operand).
__device__ __forceinline__ bf16x8_t tr8(const uint16_t* tile, int row0, const LdsOffsets& o, int s, int dblk) {
  const uint16_t* t = tile + row0 * D;
  const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(t + o.tr[s][dblk][0]));
  const bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(t + o.tr[s][dblk][1]));
  bf16x8_t out;
  out[0] = lo[0]; out[1] = lo[1]; out[2] = lo[2]; out[3] = lo[3];
  out[4] = hi[0]; out[5] = hi[1]; out[6] = hi[2]; out[7] = hi[3];
  return out;
}

__device__ __forceinline__ bf16x8_t pack_b(const float* v, int s) {
  const uint32_t w0 = hq_pack2(v[8 * s + 0], v[8 * s + 1]), w1 = hq_pack2(v[8 * s + 2], v[8 * s + 3]);
  const uint32_t w2 = hq_pack2(v[8 * s + 4], v[8 * s + 5]), w3 = hq_pack2(v[8 * s + 6], v[8 * s + 7]);
  u32x4 u = {w0, w1, w2, w3};
  return __builtin_bit_cast(bf16x8_t, u);
}

// Q fragment pre-multiplied by c = softmax_scale·log2(e) (rounded to bf16): the score MFMA then
// yields log2-domain scores directly, and its accumulator is initialised with the per-key mask bias
// (and, in the backward, minus the per-query LSE), so no per-element scale/bias/LSE VALU remains.
// The forward and both backward kernels use the identical rounded Q·c, so P is recomputed exactly.
__device__ __forceinline__ bf16x8_t prescale8(const bf16x8_t& q, float c) {
  float f[8];
  hq_unpack8(__builtin_bit_cast(uint4, q), f);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] *= c;
  return __builtin_bit_cast(bf16x8_t, hq_pack8(f));
}

__device__ __forceinline__ int acc_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

// ---------------------------------------------------------------------------------------------- output stores
// The pair swap of the row stores: A and B are a lane's packed 4-column halves of an even and an odd 8-column
// group.  swap(vdst = A, src = B): lanes 32-63 of A trade with lanes 0-31 of B, so lane q now holds
// [own A | partner's A] = the even group and lane q+32 [partner's B | own B] = the odd one.
__device__ __forceinline__ uint4 swap_halves(uint2 A, uint2 B) {
  const auto r0 = __builtin_amdgcn_permlane32_swap(A.x, B.x, false, false);
  const auto r1 = __builtin_amdgcn_permlane32_swap(A.y, B.y, false, false);
  return make_uint4(r0[0], r1[0], r0[1], r1[1]);
}

// One 64-column output row per lane pair from two transposed 32x32 accumulators (the O / dQ / dK / dV
// layout: lane q and q+32 hold the two 4-column halves of each 8-column group) as 16-B stores (playbook
// T21): one permlane32 swap per pair of groups hands lane q the 8 columns of the even group and lane q+32
// those of the odd one — 4 dwordx4 stores per lane instead of 8 dwordx2 (the store tail is issue-bound).
__device__ __forceinline__ void store_row64(uint16_t* out, const f32x16_t (&a)[2], float mul, int hh) {
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int g = 0; g < 4; g += 2) {
      const float va[4] = {a[d][4 * g] * mul, a[d][4 * g + 1] * mul, a[d][4 * g + 2] * mul, a[d][4 * g + 3] * mul};
      const float vb[4] = {a[d][4 * g + 4] * mul, a[d][4 * g + 5] * mul, a[d][4 * g + 6] * mul, a[d][4 * g + 7] * mul};
      *reinterpret_cast<uint4*>(out + d * 32 + 8 * g + 8 * hh) = swap_halves(hq_pack4(va), hq_pack4(vb));
    }
}

// A wave's 32 output rows × 64 bf16 (the same two transposed accumulators as store_row64, × mul per lane) as
// FULL 128-B lines: lane (q, hh) holds a[d][4G + j] of row q, column d·32 + 8G + 4hh + j; it writes those as
// 8-B pieces into a private 4 KiB LDS region (row r's 16-B chunk c at c ^ (r & 7): conflict-free reads), reads
// back 16 B of row (l >> 3) + 8i, chunk l & 7, and each store instruction writes 8 rows × one whole line.
// store_row64's pieces cover a quarter line per row and instruction (the GEMMs measured half-line stores
// 2-3 % slower than whole lines, profiles/r6_lines).  Rows >= nvalid are not stored.  `lds` must be free of
// other waves' traffic; the region is reused at once by the same wave (its LDS operations run in order).
constexpr int LINES_BYTES = 32 * 128;    // the region of one wave
__device__ __forceinline__ void store_tile64_lines(uint16_t* out0, size_t ld, int nvalid, const f32x16_t (&a)[2],
                                                   float mul, int lane, char* lds) {
  const int q = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int G = 0; G < 4; ++G) {
      const float v[4] = {a[d][4 * G] * mul, a[d][4 * G + 1] * mul, a[d][4 * G + 2] * mul, a[d][4 * G + 3] * mul};
      const int c = d * 4 + G;
      *reinterpret_cast<uint2*>(lds + q * 128 + ((c ^ (q & 7)) << 4) + hh * 8) = hq_pack4(v);
    }
  const int c = lane & 7, r0 = lane >> 3;
  uint4 w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = *reinterpret_cast<const uint4*>(lds + (r0 + 8 * i) * 128 + ((c ^ r0) << 4));
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (r0 + 8 * i < nvalid) *reinterpret_cast<uint4*>(out0 + (size_t)(r0 + 8 * i) * ld + c * 8) = w[i];
}

// store_row64 plus the same 8 bf16-rounded values per lane as e4m3 (x·inv8) at out8 (same element
// offsets, one byte each); returns this lane's |max| for the delayed-scaling amax.
__device__ __forceinline__ float store_row64_q8(uint16_t* out, uint8_t* out8, const f32x16_t (&a)[2], float mul,
                                                float inv8, int hh) {
  float amax = 0.f;
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int g = 0; g < 4; g += 2) {
      const float va[4] = {a[d][4 * g] * mul, a[d][4 * g + 1] * mul, a[d][4 * g + 2] * mul, a[d][4 * g + 3] * mul};
      const float vb[4] = {a[d][4 * g + 4] * mul, a[d][4 * g + 5] * mul, a[d][4 * g + 6] * mul, a[d][4 * g + 7] * mul};
      const uint4 w = swap_halves(hq_pack4(va), hq_pack4(vb));
      const int col = d * 32 + 8 * g + 8 * hh;
      *reinterpret_cast<uint4*>(out + col) = w;
      float f[8];
      hq_unpack8(w, f);   // quantise the bf16-rounded ctx, exactly what the bf16 copy holds
#pragma unroll
      for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(f[e]));
      *reinterpret_cast<uint2*>(out8 + col) = make_uint2(hq_pack_fp8x4(f, inv8), hq_pack_fp8x4(f + 4, inv8));
    }
  return amax;
}

// store_row64 plus an e5m2 copy (x·inv8) at out8 for the backward's dQ / dK / dV (the fp8 QKV dgrad's
// input), quantised from the fp32 values (one rounding; the bf16 copy is rounded separately): the four
// fp8 bytes of each 4-column half are packed BEFORE the permlane32 swap, so one swap of one dword places
// them like the bf16 words.  Saturation (only needed when this step's amax outgrew the delayed scale's 64×
// headroom) runs as a wave-uniform branch.  Returns this lane's |max| for the amax.
__device__ __forceinline__ uint32_t bf8x4_raw(float a, float b, float c, float d) {
  const uint32_t w = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, 0, false);
  return __builtin_amdgcn_cvt_pk_bf8_f32(c, d, w, true);
}
template <bool WB = true>   // WB = false: the e5m2 copy only (no bf16 output)
__device__ __forceinline__ float store_row64_e5(uint16_t* out, uint8_t* out8, const f32x16_t (&a)[2], float mul,
                                                float inv8, int hh) {
  float amax = 0.f;   // of the scaled values (|x·mul| = |x|·|mul|)
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int r = 0; r < 16; r += 2) amax = fmaxf(amax, fmaxf(fabsf(a[d][r]), fabsf(a[d][r + 1])));
  amax *= fabsf(mul);
  // rare: this step's amax outgrew the scale's 64× headroom — the fp8 copy saturates to ±57344 (e5m2 would
  // overflow to inf); the bf16 copy is unaffected
  const bool sat = __any(amax * inv8 >= kHqBf8Max);
  const float lim = kHqBf8Max / inv8;
  auto q = [&](float x) { return (sat ? fminf(fmaxf(x, -lim), lim) : x) * inv8; };
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int g = 0; g < 4; g += 2) {
      const float va[4] = {a[d][4 * g] * mul, a[d][4 * g + 1] * mul, a[d][4 * g + 2] * mul, a[d][4 * g + 3] * mul};
      const float vb[4] = {a[d][4 * g + 4] * mul, a[d][4 * g + 5] * mul, a[d][4 * g + 6] * mul, a[d][4 * g + 7] * mul};
      const int col = d * 32 + 8 * g + 8 * hh;
      if constexpr (WB) *reinterpret_cast<uint4*>(out + col) = swap_halves(hq_pack4(va), hq_pack4(vb));
      const uint32_t A8 = bf8x4_raw(q(va[0]), q(va[1]), q(va[2]), q(va[3]));
      const uint32_t B8 = bf8x4_raw(q(vb[0]), q(vb[1]), q(vb[2]), q(vb[3]));
      const auto r8 = __builtin_amdgcn_permlane32_swap(A8, B8, false, false);
      *reinterpret_cast<uint2*>(out8 + col) = make_uint2(r8[0], r8[1]);
    }
  return amax;
}

// --precision fp8, calibrated: the QKV bias gradient Σ_t dQKV[t, :] as per-wave column partials (the
// fp8 QKV weight gradient has no fused bias).  Column sums of one 32-column half of a transposed 32x32
// accumulator over the 32 lanes of each wave half (the wave's 32 tokens), as a reduce-scatter butterfly on
// VALU lane exchanges only (no LDS): lane bit 4 with v_permlane16_swap (one swap hands each 16-lane row the
// other row's half, so keep + partner = both results summed), then DPP row_ror:8 (bit 3), row_half_mirror
// (lane ^ 7: decides bit 2), quad_perm (lane ^ 2), and a final lane ^ 1 add.  Lanes l and l^1 end with the
// sum of accumulator row r = (l >> 1) & 15.  Invalid lanes (tokens past L) contribute 0.
__device__ __forceinline__ float dpp_f(float x, int ctrl_sel) {
  const int v = __float_as_int(x);
  int r;
  switch (ctrl_sel) {   // compile-time after inlining
    case 0: r = __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false); break;   // row_ror:8  (lane ^ 8)
    case 1: r = __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false); break;   // row_half_mirror (^ 7)
    case 2: r = __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false); break;    // quad_perm 2,3,0,1 (^ 2)
    default: r = __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false); break;   // quad_perm 1,0,3,2 (^ 1)
  }
  return __int_as_float(r);
}
// lanes in the (compile-time) EXEC-shaped `mask` take a, the others b: one v_cndmask_b32 on an SGPR-pair constant.
// Written as asm because hipcc rewrites the butterfly's `up ? v[i] : v[i + k]` (up = a lane bit) into a
// lane-dependent array index and lowers every such read to a 16-way v_cmp / v_cndmask chain (profiled: the
// MODE 2 dK/dV epilogue was 2,500 VALU + 750 s_nop per wave, +83 µs per layer at B = 256, L = 384)
__device__ __forceinline__ float lane_sel(uint64_t mask, float a, float b) {
  float r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(mask));
  return r;
}
__device__ __forceinline__ float colsum16(const f32x16_t& a, float mul, bool valid) {
  float v[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = valid ? a[r] * mul : 0.f;
  // bit 4: rows 0/1 (and 2/3) of 16 lanes trade halves; afterwards both hold keep + partner's
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const auto t = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[i]), __float_as_uint(v[i + 8]), false, false);
    v[i] = __uint_as_float(t[0]) + __uint_as_float(t[1]);
  }
  // bits 3, 2, 1: keep the half selected by the lane bit, add the partner's copy of it
#pragma unroll
  for (int lvl = 0; lvl < 3; ++lvl) {
    const int k = 4 >> lvl;
    // lanes with bit (8 >> lvl) set: 0xFF00…, 0xF0F0…, 0xCCCC…
    const uint64_t up = lvl == 0 ? 0xFF00FF00FF00FF00ull : lvl == 1 ? 0xF0F0F0F0F0F0F0F0ull : 0xCCCCCCCCCCCCCCCCull;
#pragma unroll
    for (int i = 0; i < k; ++i) {
      const float send = lane_sel(up, v[i], v[i + k]);
      const float keep = lane_sel(up, v[i + k], v[i]);
      v[i] = keep + dpp_f(send, lvl);
    }
  }
  return v[0] + dpp_f(v[0], 3);
}
// both halves of a row-of-64 accumulator pair -> row `dst` (64 floats: column d·32 + acc_row(r, hh))
__device__ __forceinline__ void colsum_row64(float* dst, const f32x16_t (&a)[2], float mul, bool valid, int lane,
                                             int hh) {
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const float sum = colsum16(a[d], mul, valid);
    if ((lane & 1) == 0) dst[d * 32 + acc_row((lane >> 1) & 15, hh)] = sum;
  }
}

// ------------------------------------------------------------------------------------- keep bits, lane exchanges
// x if bit `pos` of w is set, else +0: v_bfe_i32 sign-extends the bit to an all-ones / all-zero word and one
// v_and_b32 applies it (2 VALU per element instead of a bit test, a compare and a select)
__device__ __forceinline__ float keep_and(float x, uint32_t w, int pos) {
  return __uint_as_float(__float_as_uint(x) & (uint32_t)__builtin_amdgcn_sbfe((int)w, (unsigned)pos, 1u));
}
// bit of the forward's 16-bit keep word that holds element r of a lane's 16 (even elements in the low byte,
// odd in the high: the forward builds them as packed-pair flags, see attn_fwd_ring_kernel)
__host__ __device__ constexpr int kbit(int r) { return ((r & 1) << 3) | (r >> 1); }

// lane ^ 32 exchange without LDS: v_permlane32_swap hands each half the other half's value.
__device__ __forceinline__ float xor32_max(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xor32_sum(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// max over the 16 accumulator registers as a v_max3 chain
__device__ __forceinline__ float max16(const f32x16_t& a) {
  float m = fmaxf(fmaxf(a[0], a[1]), a[2]);
#pragma unroll
  for (int r = 3; r < 15; r += 2) m = fmaxf(fmaxf(m, a[r]), a[r + 1]);
  return fmaxf(m, a[15]);
}

// ------------------------------------------------------------------------------- the augmented (5th MFMA) words
__device__ __forceinline__ uint16_t bf16_rne(float f) { return (uint16_t)(hq_pack2(f, 0.f) & 0xFFFFu); }
// A key's mask bias in the log2 domain, bl = bias·log2e, as bf16 hi + bf16 lo (~16 bits): b_hi | b_lo << 16.  For a
// key past L (`live` false) the caller passes a FINITE −1e30 (exp2 → 0; no low word): lanes whose operand holds these
// words as k-dims that meet zeros on the other side compute finite × 0 = 0, where −inf × 0 would be NaN.  (The load
// of the bias stays with the caller: inside this function it changed the forward and dQ kernels' code.)
__device__ __forceinline__ uint32_t bias_word(float bl, bool live) {
  const uint16_t hi = bf16_rne(bl);
  const uint16_t lo = live ? bf16_rne(bl - hq_bf2f(hi)) : 0;
  return (uint32_t)hi | ((uint32_t)lo << 16);
}
// x (the backward's −LSE, log2 domain) to ~24 bits as three bf16
__device__ __forceinline__ void split3(float x, uint16_t& hi, uint16_t& mid, uint16_t& lo) {
  hi = bf16_rne(x);
  const float r = x - hq_bf2f(hi);
  mid = bf16_rne(r);
  lo = bf16_rne(r - hq_bf2f(mid));
}

// ------------------------------------------------------------------------------------ the K/V ring (forward, dQ)
// The head's K and V stream through an RNS-slot LDS ring of 32-key tiles by LDS-DMA (global_load_lds, 1 KiB per
// wave-instruction, source-swizzled so the lane-linear image is the conflict-free lds_off layout), RAHEAD tiles
// ahead of the consumer, with a COUNTED vmcnt + raw s_barrier per tile.  RNS = RAHEAD + 2: tiles kt … kt+RAHEAD in
// flight plus one being drained.  LDS of a workgroup: [RNS][K 4 KB | V 4 KB] | sA [Lp] of WORD | sM (dQ's dropout
// words [RW][n32][64] u16); the forward's Q staging block [RQ][64] bf16 aliases slots RAHEAD, RAHEAD+1, which are
// first restaged after the first barrier.
template <int RAHEAD, typename WORD>
struct RingLds {
  static constexpr int RNS = RAHEAD + 2;
  static constexpr int SLOT = 2 * RTILE;   // K tile | V tile
  static constexpr int sQ = RAHEAD * SLOT, sA = RNS * SLOT;
  __host__ __device__ static constexpr size_t sM(int Lp) { return sA + Lp * sizeof(WORD); }
  __host__ __device__ static constexpr size_t bytes(int Lp, int n32 = 0, bool drop = false) {
    return sM(Lp) + (drop ? (size_t)RW * n32 * 64 * sizeof(uint16_t) : 0);
  }
};

// LDS-DMA of 8 rows × 128 B (rows row0..row0+7 of `src`, ld elements apart) into a lane-linear
// [rows][64] image at `dst` (wave-uniform); the source chunk is pre-swizzled so the image is lds_off().
// Inline asm on purpose (cdna_hip_programming.md §5.7): with the builtin, hipcc treats the DMA as a
// pending LDS write and drains it (vmcnt(0)) before every later ds_read_b64_tr_b16 — which would wait
// for the tiles being prefetched.  Completion is counted by hand (vmcnt(N) + barrier per tile).
__device__ __forceinline__ void dma_piece(const uint16_t* g, char* dst) {
  const uint32_t lds = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(al_void*)dst);
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(g), "s"(lds)
      : "memory");
}
// element offset of this lane's 16 B inside an 8-row piece starting at image row row0 (source-swizzled)
__device__ __forceinline__ int dma_lane_off(int row0, size_t ld, int lane) {
  const int r = row0 + (lane >> 3);
  return (lane >> 3) * (int)ld + (((lane & 7) ^ swz(r)) << 3);
}
__device__ __forceinline__ void dma_rows8(const uint16_t* src, size_t ld, int row0, int rows_valid, char* dst,
                                          int lane) {
  const int r = row0 + (lane >> 3);
  const int rs = r < rows_valid ? r : rows_valid - 1;   // clamp: padded keys are masked by bias = -inf
  dma_piece(src + (size_t)rs * ld + (((lane & 7) ^ swz(r)) << 3), dst + row0 * 128);
}

// `vmcnt(n)` with a value that constant-folds once the tile loop is unrolled
__device__ __forceinline__ void wait_vm(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
  }
}

// tile kt → slot kt % RNS: this wave's K and V piece (8 rows each).  kv_off = dma_lane_off(wave·8) + wave·8·ld.
// FULL: every tile has 32 keys (L % 32 == 0), which also selects the unclamped DMA addressing.
template <typename LDS, bool FULL>
__device__ __forceinline__ void kv_stage(char* ring, const uint16_t* base, int H, int ld, int L, int kv_off, int wave,
                                         int lane, int kt) {
  char* slot = ring + (kt % LDS::RNS) * LDS::SLOT;
  const uint16_t* kb = base + H + (size_t)kt * 32 * ld;   // wave-uniform
  if (FULL || kt * 32 + 32 <= L) {
    dma_piece(kb + kv_off, slot + wave * 8 * 128);
    dma_piece(kb + H + kv_off, slot + RTILE + wave * 8 * 128);
  } else {
    dma_rows8(kb, ld, wave * 8, L - kt * 32, slot, lane);
    dma_rows8(kb + H, ld, wave * 8, L - kt * 32, slot + RTILE, lane);
  }
}
// tile kt landed: wait until only `extra` younger memory operations of the caller's and the two DMA pieces of each
// later staged tile are outstanding.  Iteration j stages tile j + RAHEAD (if it exists), so the stages younger than
// tile kt's are those of iterations kt − RAHEAD + 1 … kt − 1 that exist (prologue tiles kt < RAHEAD were drained
// before the loop: any count is safe for them).
template <int RAHEAD>
__device__ __forceinline__ void kv_wait(int kt, int n32, int extra) {
  const int later = kt + RAHEAD - 1 < n32 ? RAHEAD - 1 : n32 - 1 - kt;
  wait_vm(extra + 2 * (later > 0 ? later : 0));
}

// ------------------------------------------------------------------------------------------------------ dK/dV LDS
// Two slots, one per 32-query tile in flight; dV / dK leave through the same memory (store_tile64_lines, one
// region per wave) once the last tile is consumed.
struct DkvLds {
  static constexpr int Q = 0;                                        // Q' = Q·c [32][64] bf16
  static constexpr int DO = Q + RTILE;                               // dO [32][64] bf16
  static constexpr int AW = DO + RTILE;                              // A' words [32] uint4
  static constexpr int DELTA = AW + 32 * sizeof(uint4);              // δ [32] f32
  static constexpr int BITS = DELTA + 32 * sizeof(float);            // dropout words [RW][64] u16
  static constexpr int SLOT = BITS + RW * 64 * sizeof(uint16_t);
  __host__ __device__ static constexpr int slot(int t) { return (t & 1) * SLOT; }
  __host__ __device__ static constexpr size_t bytes() { return 2 * (size_t)SLOT; }
  static_assert(2 * SLOT >= RW * LINES_BYTES, "dK/dV store staging: one region per wave in the two slots");
};

// ------------------------------------------------------------------------------------------------------ launchers
// run(std::integral_constant<int, NT>): NT = L / 32 for the lengths whose tile loop is fully unrolled, else 0 (the
// rolled loop, any L <= 512).  NT > 0 implies L = 32·NT, so the kernels' ragged variants (clamped DMA addressing,
// the forward's EVEN = false) exist only for NT = 0: never select an unclamped one for a ragged L.
template <typename F>
void dispatch_nt(int L, F&& run) {
  if (L == 384) run(std::integral_constant<int, 12>{});
  else if (L == 512) run(std::integral_constant<int, 16>{});
  else if (L == 256) run(std::integral_constant<int, 8>{});
  else if (L == 128) run(std::integral_constant<int, 4>{});
  else run(std::integral_constant<int, 0>{});
}

}  // namespace
