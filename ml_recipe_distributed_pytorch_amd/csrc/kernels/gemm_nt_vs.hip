// bf16 NT GEMM, vS — 128×128 tiles for the shapes the 256-row kernels do not cover well: M % 256 != 0 (dynamically
// padded NQ batches, the reference micro-batch of 2 × 512 tokens) and grids that fill the 256 CUs
// poorly with 256² tiles (batch 64: N = 768 gives 288 tiles = 1.1 waves).  4 waves (2 M × 2 N, 64×64
// each), two 32 KiB LDS-DMA stages (buffer_load … lds, same source swizzle as the big kernels), so two
// workgroups share a CU.  The M tail costs nothing extra: the A descriptor's num_records ends at row M,
// the out-of-range rows stage as zeros, and the epilogue stores only rows < M.  Same epilogues as v1;
// DGELU / DMUL column partials are per 128-row block (part has ceil(M/128) rows).
// Split-K (ksplit > 1, EPI none / bias / resid only): for grids far below one workgroup per CU with a long
// K (the reference micro-batch of 2 × 512 tokens: 48 tiles of N = 768 at K = 3072 / 2304), workgroup
// id / tiles sums K-tiles [split·nt/ksplit, (split+1)·nt/ksplit) into fp32 slab ws[split] and
// splitk_epi_kernel folds the slabs in order (deterministic) and applies the epilogue.
#include <algorithm>
#include <cstdlib>

#include "hq_gemm_epi.h"
#include "hq_gemm_nt.h"
#include "hq_gemm_tile.h"

namespace {

using namespace hq_tile;

// split-K: only the epilogues without column partials, GELU or dropout (none / bias / resid)
constexpr bool nts_can_split(int epi) { return !hq_epi_col_partials(epi) && !hq_epi_writes_p(epi) && epi != HQ_EPI_BDR; }

template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_nts_kernel(const uint16_t* __restrict__ A, const uint16_t* __restrict__ B,
                                                          uint16_t* __restrict__ C, const float* __restrict__ bias,
                                                          uint16_t* __restrict__ P, const uint16_t* __restrict__ R,
                                                          float* __restrict__ part, int M, int N, int K, int lda, int ldb,
                                                          int ldc, int ksplit, float* __restrict__ ws, HqDropArg dr) {
  const uint32_t key = EPI == HQ_EPI_BDR ? dr.kd.get() : 0u;   // EPI_BDR dropout key (device seed word under graphs)
  constexpr int SB = 128;                  // tile rows = tile cols
  constexpr int PANEL = SB * 128;          // one operand panel: 128 rows × 64 bf16
  constexpr int STAGE = 2 * PANEL;
  constexpr int RS = 64 * 2 + 16;          // epilogue staging row stride (bytes)
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int wm = wave >> 1, wn = wave & 1;

  const int nwg = gridDim.x, id = hq_xcd_tile(blockIdx.x, nwg);
  const int tiles = nwg / ksplit;
  const int split = id / tiles, tile = id - split * tiles;
  const int tiles_n = N / SB;
  const int tm = tile / tiles_n, tn = tile % tiles_n;
  const int m0 = tm * SB, n0 = tn * SB;
  const int rows_a = min(SB, M - m0);
  const int nk = K / BK, kt0 = split * nk / ksplit, nt = (split + 1) * nk / ksplit - kt0;
  HQ_DASSERT(rows_a > 0 && n0 + SB <= N && K % BK == 0 && nt > 0 && (ksplit == 1 || nts_can_split(EPI)));

  const __amdgpu_buffer_rsrc_t ra =
      __builtin_amdgcn_make_buffer_rsrc((void*)(A + (size_t)m0 * lda), (short)0, rows_a * lda * 2, kRawBufferWord3);
  const __amdgpu_buffer_rsrc_t rb =
      __builtin_amdgcn_make_buffer_rsrc((void*)(B + (size_t)n0 * ldb), (short)0, SB * ldb * 2, kRawBufferWord3);
  int voA[4], voB[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {   // wave w stages rows w·32 … +31 of each panel
    const int row0 = wave * 32 + i * 8;
    voA[i] = lane_src_offset(row0, lane, lda);
    voB[i] = lane_src_offset(row0, lane, ldb);
  }
  auto stage = [&](int t, int buf) {
    char* base = smem + buf * STAGE + wave_u * 32 * 128;
    const int ko = (kt0 + t) * BK * 2;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void*)(base + i * 8 * 128), 16, voA[i], ko, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (lds_void*)(base + PANEL + i * 8 * 128), 16, voB[i], ko, 0, 0);
  };

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fq = lane >> 4;
  stage(0, 0);
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) {
      stage(t + 1, (t + 1) & 1);
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");   // this wave's 8 pieces of stage t landed
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    bar();                                               // ... and every other wave's
    const char* pa = smem + (t & 1) * STAGE;
    const char* pb = pa + PANEL;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t af[4], bf[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) bf[j] = frag(pb, wn * 64 + j * 16 + fr, ks * 4 + fq);
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = frag(pa, wm * 64 + i * 16 + fr, ks * 4 + fq);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(bf[j], af[i], acc[i][j]);
      __builtin_amdgcn_s_setprio(0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    bar();                                               // WAR: stage t+2 reuses this buffer
  }

  if (ksplit > 1) {   // fp32 slab of this split: lane holds C[m][n … n+3] (swapped-operand accumulator)
    float* slab = ws + (size_t)split * M * N;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wm * 64 + i * 16 + fr;
      if (m >= M) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4_t& a = acc[i][j];
        *reinterpret_cast<float4*>(slab + (size_t)m * N + n0 + wn * 64 + j * 16 + fq * 4) =
            make_float4(a[0], a[1], a[2], a[3]);
      }
    }
    return;
  }

  // ---- epilogue: acc (+bias) -> bf16 in this wave's LDS region [64][64], then row-coalesced 16-B pieces
  char* wreg = smem + wave * 64 * RS;
  constexpr bool kBias = hq_epi_has_bias(EPI);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int nl = j * 16 + fq * 4;
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (kBias) bv = *reinterpret_cast<const float4*>(bias + n0 + wn * 64 + nl);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v[4] = {acc[i][j][0] + bv.x, acc[i][j][1] + bv.y, acc[i][j][2] + bv.z, acc[i][j][3] + bv.w};
      *reinterpret_cast<uint2*>(wreg + (i * 16 + fr) * RS + nl * 2) = hq_pack4(v);
    }
  }
  constexpr int SEGS = 8, ROWS_PER_IT = 64 / SEGS;
  const int seg = lane % SEGS, rsub = lane / SEGS;
  const int gcol = n0 + wn * 64 + seg * 8;
  const uint16_t* aux_src = hq_epi_col_partials(EPI) ? P : R;
  float csum[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) csum[e] = 0.f;
#pragma unroll 2
  for (int it = 0; it < 64 / ROWS_PER_IT; ++it) {
    const int row = it * ROWS_PER_IT + rsub;
    const int grow = m0 + wm * 64 + row;
    if (grow >= M) continue;
    uint4 piece = *reinterpret_cast<const uint4*>(wreg + row * RS + seg * 16);
    const size_t goff = (size_t)grow * ldc + gcol;
    hq_epi_piece<EPI>(piece, [&]() -> const uint4& { return *reinterpret_cast<const uint4*>(aux_src + goff); }, goff, dr,
                      key, csum, [&](const uint4& p) { *reinterpret_cast<uint4*>(P + goff) = p; });
    *reinterpret_cast<uint4*>(C + goff) = piece;
  }
  if constexpr (hq_epi_col_partials(EPI)) {
    hq_epi_csum_reduce<SEGS>(csum);
    float* red = reinterpret_cast<float*>(smem + 4 * 64 * RS);  // [2][128], past the staging regions
    if (rsub == 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) red[wm * SB + wn * 64 + seg * 8 + e] = csum[e];
    }
    __syncthreads();
    if (tid < SB) part[(size_t)tm * N + n0 + tid] = red[tid] + red[SB + tid];
  }
}

// C[m, n] = epi(Σ_s ws[s][m][n]) for the split-K vS path: slabs summed in split order (deterministic).
template <int EPI>
__global__ __launch_bounds__(256) void splitk_epi_kernel(const float* __restrict__ ws, int ksplit, uint16_t* __restrict__ C,
                                                         const float* __restrict__ bias, const uint16_t* __restrict__ R,
                                                         int M, int N, int ldc) {
  const size_t n8 = (size_t)M * N / 8;
  for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
    const size_t e = i * 8;
    const int m = (int)(e / N), n = (int)(e - (size_t)m * N);
    float v[8];
    const float4* w0 = reinterpret_cast<const float4*>(ws + e);
    float4 a = w0[0], b = w0[1];
    for (int s = 1; s < ksplit; ++s) {
      const float4* ws_s = reinterpret_cast<const float4*>(ws + (size_t)s * M * N + e);
      const float4 c = ws_s[0], d = ws_s[1];
      a.x += c.x; a.y += c.y; a.z += c.z; a.w += c.w;
      b.x += d.x; b.y += d.y; b.z += d.z; b.w += d.w;
    }
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    if constexpr (EPI == HQ_EPI_BIAS) {
      const float4 b0 = *reinterpret_cast<const float4*>(bias + n), b1 = *reinterpret_cast<const float4*>(bias + n + 4);
      v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w; v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
    } else if constexpr (EPI == HQ_EPI_RESID) {
      float rr[8];
      hq_unpack8(*reinterpret_cast<const uint4*>(R + (size_t)m * ldc + n), rr);
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] += rr[k];
    }
    *reinterpret_cast<uint4*>(C + (size_t)m * ldc + n) = hq_pack8(v);
  }
}

// vS split-K factor (epilogues that can split: nts_can_split): grids below half a workgroup per CU,
// and at least 8 K-tiles per split; HQ_GEMM_SPLITK=0 disables (A/B), N > 1 forces up to N.
int g_nts_splitk = [] {
  const char* e = getenv("HQ_GEMM_SPLITK");
  return e ? atoi(e) : -1;
}();

template <int EPI>
void launch_vs(const HqNtArgs& a, float* ws, hipStream_t s) {
  constexpr size_t lds = 2 * 2 * 128 * 128;
  [[maybe_unused]] static const bool once = hq_raise_lds_limit({(const void*)gemm_nts_kernel<EPI>}, lds);
  const int grid_s = ((a.M + 127) / 128) * (a.N / 128);
  // no workspace from the caller: run unsplit rather than share a scratch buffer
  const int ks = ws ? hq_nt_vs_ksplit(EPI, grid_s, a.K / BK) : 1;
  a.launch(gemm_nts_kernel<EPI>, grid_s * ks, 256, lds, s, ks, ws);
  if (ks > 1) {
    const size_t n8 = (size_t)a.M * a.N / 8;
    const int g = (int)std::min<size_t>((n8 + 255) / 256, 2048);
    hipLaunchKernelGGL((splitk_epi_kernel<nts_can_split(EPI) ? EPI : HQ_EPI_NONE>), dim3(g), dim3(256), 0, s, ws, ks, a.C,
                       a.bias, a.R, a.M, a.N, a.ldc);
  }
}

}  // namespace

int hq_nt_vs_ksplit(int epi, int tiles, int nk) {
  if (!nts_can_split(epi) || g_nts_splitk == 0) return 1;
  int ks = g_nts_splitk > 1 ? g_nts_splitk : (2 * tiles <= hq_num_cus() ? 2 * hq_num_cus() / tiles : 1);
  ks = std::min(ks, std::min(4, nk / 8));
  return ks > 1 ? ks : 1;
}

void hq_nt_vs_launch(int epi, const HqNtArgs& a, float* ws, hipStream_t s) {
  hq_with_epi(epi, [&](auto e) { launch_vs<decltype(e)::value>(a, ws, s); });
}
