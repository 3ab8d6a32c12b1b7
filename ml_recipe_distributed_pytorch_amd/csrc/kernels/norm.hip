// LayerNorm of the BERT encoder (gfx950, wave64).
//
//   ln_fwd   : z = dropout(a) + resid (rounded to bf16, as HF under autocast) ; y = LN(z)
//   ln_bwd   : dz = LN_bwd(dy [+ dy2]) ; da = dropout_bwd(dz) ; per-block partial Σ(g·x̂), Σg, Σda
//   ln_guard : which LayerNorms may recompute x̂ from their output y
//
// Layout: one wave per row; lane owns 4 consecutive columns per 256-column chunk (8-byte bf16
// vector access), NCH = ceil(H/256) chunks.  Column partial sums are reduced per block through
// LDS and finished by hq_colsum_outs (rowops.hip: one 1024-thread block per 64 columns), so every gradient is
// bitwise deterministic.

#include "hq_common.h"
#include "hq_kernels.h"
#include "hq_rowops.h"

namespace {

// LayerNorm forward, RPW rows per wave.  RES = true: z = dropout(a) + resid (rounded to bf16, as HF under
// autocast; stored only when z != null — the backward recomputes x̂ from y) ; y = LN(z).  RES = false: y =
// LN(z) where z was already written by the producing GEMM's EPI_BDR epilogue (out-projection / FFN2).
// Each wave issues all its rows' loads before the first reduction: one row per wave was latency-bound
// (88.7 µs at T = 98304 with RES, 5.1 TB/s over its three streams; RPW = 2: 77.7 µs, 5.8 TB/s; RPW = 4
// 84.0 µs — profiles/r3_ln_rpw).
// Q8 (--precision fp8): y is also written as e4m3 under the delayed scale of the consuming GEMM's input
// state q8 (the next QKV / FFN1 projection reads it instead of a separate quantisation pass over y).  Each
// wave's amax goes to a partial slot that hq_fp8_amax_fold reduces (no same-address atomics: those
// serialise in one L2 channel — a per-block filtered atomic cost +27 µs at T = 98304, a per-wave one +97).
template <int NCH, int RPW, bool RES, bool Q8 = false>
__global__ __launch_bounds__(256) void ln_fwd_rows_kernel(const uint16_t* __restrict__ zin, const uint16_t* __restrict__ resid,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          uint16_t* __restrict__ y, uint16_t* __restrict__ z,
                                                          float* __restrict__ mean_out, float* __restrict__ rstd_out, int T,
                                                          int H, float eps, HqDropKey kd_, uint32_t thr, float kscale,
                                                          uint8_t* __restrict__ y8, const float* __restrict__ q8,
                                                          float* __restrict__ part8, int phase) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float amax = 0.f, inv8 = 1.f;
  if constexpr (Q8) {
    hq_fp8_publish_scale(q8, phase);
    inv8 = 1.f / hq_fp8_delayed_scale(q8, phase);
  }
  const int row0 = (blockIdx.x * kWaves + wave) * RPW;
  uint2 ra[RPW][NCH], rr[RES ? RPW : 1][NCH];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int col = c * 256 + lane * 4;
      const bool ok = row0 + r < T && col < H;
      const size_t off = (size_t)(row0 + r) * H + col;
      ra[r][c] = ok ? *reinterpret_cast<const uint2*>(zin + off) : make_uint2(0u, 0u);
      if constexpr (RES) rr[r][c] = ok ? *reinterpret_cast<const uint2*>(resid + off) : make_uint2(0u, 0u);
    }
  float v[RPW][NCH][4];
  if constexpr (RES) {
    const uint32_t key = kd_.get();
#pragma unroll
    for (int r = 0; r < RPW; ++r)
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int col = c * 256 + lane * 4;
        const size_t off = (size_t)(row0 + r) * H + col;
        float fa[4], fr[4], m[4] = {1.f, 1.f, 1.f, 1.f};
        hq_unpack4(ra[r][c], fa);
        hq_unpack4(rr[r][c], fr);
        if (thr) hq_keep4((uint32_t)off, key, thr, kscale, m);
        float zz[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) zz[i] = fa[i] * m[i] + fr[i];
        const uint2 packed = hq_pack4(zz);
        if (z && row0 + r < T && col < H) *reinterpret_cast<uint2*>(z + off) = packed;
        hq_unpack4(packed, v[r][c]);   // statistics of the bf16-rounded z
      }
  } else {
#pragma unroll
    for (int r = 0; r < RPW; ++r)
#pragma unroll
      for (int c = 0; c < NCH; ++c) hq_unpack4(ra[r][c], v[r][c]);
  }
  float mean[RPW], rstd[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) sum += v[r][c][i];
    mean[r] = hq_wave_sum(sum) / H;
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int col = c * 256 + lane * 4;
      if (col < H) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float d = v[r][c][i] - mean[r]; sq += d * d; }
      }
    }
    rstd[r] = rsqrtf(hq_wave_sum(sq) / H + eps);
  }
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 256 + lane * 4;
    if (col < H) {
      const float4 g = *reinterpret_cast<const float4*>(gamma + col);
      const float4 b = *reinterpret_cast<const float4*>(beta + col);
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        if (row0 + r < T) {
          float o[4] = {(v[r][c][0] - mean[r]) * rstd[r] * g.x + b.x, (v[r][c][1] - mean[r]) * rstd[r] * g.y + b.y,
                        (v[r][c][2] - mean[r]) * rstd[r] * g.z + b.z, (v[r][c][3] - mean[r]) * rstd[r] * g.w + b.w};
          const uint2 packed = hq_pack4(o);
          *reinterpret_cast<uint2*>(y + (size_t)(row0 + r) * H + col) = packed;
          if constexpr (Q8) {
            hq_unpack4(packed, o);   // quantise the bf16-rounded y, exactly what the bf16 copy holds
#pragma unroll
            for (int i = 0; i < 4; ++i) amax = fmaxf(amax, fabsf(o[i]));
            *reinterpret_cast<uint32_t*>(y8 + (size_t)(row0 + r) * H + col) = hq_pack_fp8x4(o, inv8);
          }
        }
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < RPW; ++r)
      if (row0 + r < T) { mean_out[row0 + r] = mean[r]; rstd_out[row0 + r] = rstd[r]; }
  }
  if constexpr (Q8) {   // this wave's amax -> its own partial slot
    amax = hq_wave_max(amax);
    if (lane == 0) part8[blockIdx.x * kWaves + wave] = amax;
  }
}

// Rows of one wave are software-pipelined: the next row's dy/dy2/z loads are in flight while the
// current row is reduced and stored (the kernel is HBM-latency bound at 3 waves/SIMD otherwise).
template <int NCH>
__device__ __forceinline__ void ln_bwd_load(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ dy2,
                                            const uint16_t* __restrict__ z, size_t base, int lane, int H,
                                            uint2 (&vdy)[NCH], uint2 (&vdy2)[NCH], uint2 (&vz)[NCH]) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 256 + lane * 4;
    if (col < H) {
      vdy[c] = *reinterpret_cast<const uint2*>(dy + base + col);
      vdy2[c] = dy2 ? *reinterpret_cast<const uint2*>(dy2 + base + col) : make_uint2(0u, 0u);
      vz[c] = *reinterpret_cast<const uint2*>(z + base + col);
    }
  }
}

// RPW rows per wave: 8 at large T (partials amortised), 2 for small token counts (T = 1024: 32 blocks of
// 8-row waves left most CUs idle and each wave latency-bound — see ln_rows_per_wave)
// FROMY ("memory-efficient" LayerNorm backward): the third input is the forward OUTPUT y instead of z, and
// x̂ = (y − β)/γ = y·(1/γ) − β/γ per column (one FMA) — the forward then never stores z (151 MB per LayerNorm at
// T = 98304), and rstd is the only row statistic read.  x̂ carries y's bf16 rounding scaled by 1/γ instead of
// z's.  A column with γ = 0 has no recoverable x̂ (set to 0): its own dz (via x̂·mean(g·γ·x̂)) and γ gradient are
// then wrong — the limit of every "memory-efficient" LayerNorm; HQ_LN_FROM_Y=0 keeps z for such models.
template <int NCH, int RPW = kRowsPerWave, bool Q8 = false, bool FROMY = false>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ dy2,
                                                     const uint16_t* __restrict__ z, const float* __restrict__ gamma,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     uint16_t* __restrict__ dz_out, uint16_t* __restrict__ da_out,
                                                     float* __restrict__ part, int T, int H, HqDropKey kd_, uint32_t thr,
                                                     float kscale, uint8_t* __restrict__ da8, const float* __restrict__ q8,
                                                     float* __restrict__ part8, int phase, const float* __restrict__ beta) {
  const uint32_t key = kd_.get();
  // Q8 (--precision fp8 backward): da also as e5m2 under the delayed scale of the dgrad GEMM that consumes
  // it (state q8), so that GEMM runs on fp8 operands without a separate quantisation pass
  float inv8 = 1.f, amax8 = 0.f;
  if constexpr (Q8) {
    hq_fp8_publish_scale(q8, phase, kHqBf8Max);
    inv8 = 1.f / hq_fp8_delayed_scale(q8, phase, kHqBf8Max);
  }
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float acc[3][NCH][4];
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[q][c][i] = 0.f;
  float gam[NCH][4], ig[FROMY ? NCH : 1][4], nb[FROMY ? NCH : 1][4];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 256 + lane * 4;
    float4 g = col < H ? *reinterpret_cast<const float4*>(gamma + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    gam[c][0] = g.x; gam[c][1] = g.y; gam[c][2] = g.z; gam[c][3] = g.w;
    if constexpr (FROMY) {
      const float4 b = col < H ? *reinterpret_cast<const float4*>(beta + col) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ig[c][i] = gam[c][i] != 0.f ? 1.f / gam[c][i] : 0.f;
        nb[c][i] = -bb[i] * ig[c][i];
      }
    }
  }
  const int row0 = blockIdx.x * kWaves * RPW + wave;
  // loads run TWO rows ahead (c = this row, n = next, f = the one after): with one row in flight per
  // wave the kernel left ~15 % of the HBM bandwidth unused at its 4 waves/SIMD occupancy
  uint2 cdy[NCH], cdy2[NCH], cz[NCH], ndy[NCH], ndy2[NCH], nz[NCH];
  float cmu = 0.f, crs = 0.f, nmu = 0.f, nrs = 0.f;
  if (row0 < T) {
    ln_bwd_load<NCH>(dy, dy2, z, (size_t)row0 * H, lane, H, cdy, cdy2, cz);
    cmu = mean[row0];
    crs = rstd[row0];
  }
  if (RPW > 1 && row0 + kWaves < T) {
    ln_bwd_load<NCH>(dy, dy2, z, (size_t)(row0 + kWaves) * H, lane, H, ndy, ndy2, nz);
    nmu = mean[row0 + kWaves];
    nrs = rstd[row0 + kWaves];
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int row = row0 + r * kWaves;
    if (row < T) {
      const size_t base = (size_t)row * H;
      uint2 fdy[NCH], fdy2[NCH], fz[NCH];
      float fmu = 0.f, frs = 0.f;
      const int frow = row + 2 * kWaves;
      if (r + 2 < RPW && frow < T) {
        ln_bwd_load<NCH>(dy, dy2, z, (size_t)frow * H, lane, H, fdy, fdy2, fz);
        fmu = mean[frow];
        frs = rstd[frow];
      }
      float g[NCH][4], xh[NCH][4];
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int col = c * 256 + lane * 4;
        if (col < H) {
          float fz[4], f2[4];
          hq_unpack4(cdy[c], g[c]);
          hq_unpack4(cdy2[c], f2);
          hq_unpack4(cz[c], fz);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            g[c][i] += f2[i];
            if constexpr (FROMY) xh[c][i] = fmaf(fz[i], ig[c][i], nb[c][i]);
            else xh[c][i] = (fz[i] - cmu) * crs;
            acc[0][c][i] += g[c][i] * xh[c][i];
            acc[1][c][i] += g[c][i];
            const float dxh = g[c][i] * gam[c][i];
            s1 += dxh;
            s2 += dxh * xh[c][i];
          }
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) { g[c][i] = 0.f; xh[c][i] = 0.f; }
        }
      }
      s1 = hq_wave_sum(s1) / H;
      s2 = hq_wave_sum(s2) / H;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int col = c * 256 + lane * 4;
        if (col < H) {
          float dz[4], m[4] = {1.f, 1.f, 1.f, 1.f};
#pragma unroll
          for (int i = 0; i < 4; ++i) dz[i] = crs * (g[c][i] * gam[c][i] - s1 - xh[c][i] * s2);
          *reinterpret_cast<uint2*>(dz_out + base + col) = hq_pack4(dz);
          if (thr) hq_keep4((uint32_t)(base + col), key, thr, kscale, m);
          float da[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) { da[i] = dz[i] * m[i]; acc[2][c][i] += da[i]; }
          const uint2 da_bf = hq_pack4(da);
          // da_out == null (Q8 only, --precision fp8 once every consumer reads da8): no bf16 da
          if (!Q8 || da_out != nullptr) *reinterpret_cast<uint2*>(da_out + base + col) = da_bf;
          if constexpr (Q8) {   // from the bf16-rounded da, exactly what the bf16 copy holds
            float r[4];
            hq_unpack4(da_bf, r);
#pragma unroll
            for (int i = 0; i < 4; ++i) amax8 = fmaxf(amax8, fabsf(r[i]));
            *reinterpret_cast<uint32_t*>(da8 + base + col) = hq_pack_bf8x4(r, inv8);
          }
        }
      }
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        cdy[c] = ndy[c]; cdy2[c] = ndy2[c]; cz[c] = nz[c];
        ndy[c] = fdy[c]; ndy2[c] = fdy2[c]; nz[c] = fz[c];
      }
      cmu = nmu; crs = nrs;
      nmu = fmu; nrs = frs;
    }
  }
  if constexpr (Q8) {   // this wave's amax -> its own partial slot (hq_fp8_amax_fold reduces them)
    amax8 = hq_wave_max(amax8);
    if (lane == 0) part8[blockIdx.x * kWaves + wave] = amax8;
  }
  block_partials<NCH, 3>(acc, lds, part, H);
}

}  // namespace

// ================================================================================== launchers
void hq_ln_fwd(const uint16_t* a, const uint16_t* resid, const float* gamma, const float* beta, uint16_t* y, uint16_t* z,
               float* mean, float* rstd, int T, int H, float eps, float p, uint32_t seed, uint32_t opid, hipStream_t s,
               uint8_t* y8, float* q8, int phase) {
  const uint32_t thr = p > 0.f ? hq_threshold(p) : 0u;
  const HqDropKey key = hq_drop_key(seed, opid);
  const float ks = hq_keep_scale(thr);
  constexpr int rpw = 2;   // rows per wave (1 / 2 / 4 measured: profiles/r3_ln_rpw)
  const int grid = (T + kWaves * rpw - 1) / (kWaves * rpw);
  float* part8 = y8 ? hq_fp8_amax_parts((size_t)grid * kWaves, q8, s) : nullptr;
  dispatch_nch(H, [&](auto nch) {
    constexpr int C = decltype(nch)::value;
    auto go = [&](auto R, auto res, auto q) {
      hipLaunchKernelGGL((ln_fwd_rows_kernel<C, decltype(R)::value, decltype(res)::value, decltype(q)::value>),
                         dim3(grid), dim3(256), 0, s, a, resid, gamma, beta, y, z, mean, rstd, T, H, eps, key, thr, ks,
                         y8, q8, part8, phase);
    };
    auto by_rows = [&](auto res, auto q) {
      if (rpw == 1) go(std::integral_constant<int, 1>{}, res, q);
      else if (rpw == 4) go(std::integral_constant<int, 4>{}, res, q);
      else go(std::integral_constant<int, 2>{}, res, q);
    };
    // resid == null: a = z from an EPI_BDR GEMM epilogue
    if (y8) { if (resid) by_rows(std::true_type{}, std::true_type{}); else by_rows(std::false_type{}, std::true_type{}); }
    else if (resid) by_rows(std::true_type{}, std::false_type{});
    else by_rows(std::false_type{}, std::false_type{});
  });
  if (y8) hq_fp8_amax_fold(part8, grid * kWaves, q8, phase, s);
}

int hq_ln_rows_per_wave(int T) { return T >= 16384 ? kRowsPerWave : 2; }
int hq_ln_bwd_partials(int T) {
  const int rpw = hq_ln_rows_per_wave(T);
  return (T + kWaves * rpw - 1) / (kWaves * rpw);
}

void hq_ln_bwd(const uint16_t* dy, const uint16_t* dy2, const uint16_t* z, const float* gamma, const float* mean,
               const float* rstd, uint16_t* dz, uint16_t* da, float* part, HqOuts outs, int T, int H, float p,
               uint32_t seed, uint32_t opid, bool accumulate, hipStream_t s, uint8_t* da8, float* q8, int phase,
               const float* beta) {
  const uint32_t thr = p > 0.f ? hq_threshold(p) : 0u;
  const HqDropKey key = hq_drop_key(seed, opid);
  const float ks = hq_keep_scale(thr);
  const int nb = hq_ln_bwd_partials(T);
  float* part8 = da8 ? hq_fp8_amax_parts((size_t)nb * kWaves, q8, s) : nullptr;
  dispatch_nch(H, [&](auto nch) {
    constexpr int C = decltype(nch)::value;
    auto go = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 4 * H * sizeof(float), s, dy, dy2, z, gamma, mean, rstd, dz, da, part,
                         T, H, key, thr, ks, da8, q8, part8, phase, beta);
    };
    // beta != null: `z` is the forward output y (FROMY)
    if (hq_ln_rows_per_wave(T) == kRowsPerWave) {
      if (da8) { if (beta) go(ln_bwd_kernel<C, kRowsPerWave, true, true>); else go(ln_bwd_kernel<C, kRowsPerWave, true, false>); }
      else { if (beta) go(ln_bwd_kernel<C, kRowsPerWave, false, true>); else go(ln_bwd_kernel<C, kRowsPerWave, false, false>); }
    } else {
      if (da8) { if (beta) go(ln_bwd_kernel<C, 2, true, true>); else go(ln_bwd_kernel<C, 2, true, false>); }
      else { if (beta) go(ln_bwd_kernel<C, 2, false, true>); else go(ln_bwd_kernel<C, 2, false, false>); }
    }
  });
  if (da8) hq_fp8_amax_fold(part8, nb * kWaves, q8, phase, s, kHqBf8Max);
  hq_colsum_outs(part, nb, 3 * H, outs, H, accumulate, s);
}

// LayerNorm-from-y guard (models/bert.py _ln_flags): LayerNorm i may recompute x̂ from its bf16 output iff every
// column has γ != 0 and |β| <= ratio·|γ|.  One block per LayerNorm over the fp32 master arena (γ at goff[i], β at
// boff[i]); flags[i] = 1 / 0.  Replaces a stack / abs / compare / and / all chain of ATen kernels.
__global__ __launch_bounds__(256) void ln_guard_kernel(const float* __restrict__ master, const int64_t* __restrict__ goff,
                                                       const int64_t* __restrict__ boff, int H, float ratio,
                                                       uint8_t* __restrict__ flags) {
  const float* g = master + goff[blockIdx.x];
  const float* b = master + boff[blockIdx.x];
  int bad = 0;
  for (int c = threadIdx.x; c < H; c += 256) {
    const float ag = fabsf(g[c]), ab = fabsf(b[c]);
    bad |= !(ag > 0.f && ab <= ratio * ag);
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) flags[blockIdx.x] = bad ? 0 : 1;
}

void hq_ln_guard(const float* master, const int64_t* goff, const int64_t* boff, int n, int H, float ratio, uint8_t* flags,
                 hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(ln_guard_kernel, dim3(n), dim3(256), 0, s, master, goff, boff, H, ratio, flags);
}
