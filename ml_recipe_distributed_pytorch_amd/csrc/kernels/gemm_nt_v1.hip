// bf16 NT GEMM, v1: the whole-tile double buffer (N % 256 != 0 → 128-wide blocks, K = 64, or forced).
//
// Structure (CDNA4 playbook §5):
// * 256×BN block tile, BK = 64, 512 threads = 8 waves as 2 (M) × 4 (N); a wave owns 128 × BN/4.
// * Operands reach LDS by LDS-DMA (global_load_lds, 16 B per lane): the image is lane-linear, so the
//   bank-conflict XOR swizzle is applied to the per-lane global SOURCE address and undone on the
//   ds_read_b128 fragment read (rule 21).  Rows are 128 B; slot' = slot ^ ((row >> 1) & 7) makes the
//   16-lane fragment reads of 16 rows hit all 64 banks once.
// * Double-buffered ring: tile t+1 is issued before tile t is consumed; each wave drains its own DMA
//   (vmcnt(0)) once per K-tile, ahead of a raw s_barrier (no __syncthreads).  One __shared__ array for
//   everything (trap 4a).
// * mfma_f32_16x16x32_bf16 with the operands SWAPPED (B fragment as the MFMA's A input) so the
//   accumulator holds Cᵀ: each lane owns 4 consecutive n of one m → 8-byte row-contiguous stores,
//   a float4 of bias per lane, and the column (bias-grad) sums reduce over lanes.
// * XCD-aware bijective block remap: each XCD walks a contiguous range of tiles in M-major order,
//   so the tiles that share an A row-panel share that XCD's L2.
#include "hq_gemm_epi.h"
#include "hq_gemm_nt.h"
#include "hq_gemm_tile.h"

namespace {

using namespace hq_tile;

template <int EPI, int BN>
__global__ __launch_bounds__(kThreads, 1) void gemm_nt_kernel(const uint16_t* __restrict__ A, const uint16_t* __restrict__ B,
                                                              uint16_t* __restrict__ C, const float* __restrict__ bias,
                                                              uint16_t* __restrict__ P, const uint16_t* __restrict__ R,
                                                              float* __restrict__ part, int M, int N, int K, int lda,
                                                              int ldb, int ldc, HqDropArg dr) {
  const uint32_t key = EPI == HQ_EPI_BDR ? dr.kd.get() : 0u;   // EPI_BDR dropout key (device seed word under graphs)
  constexpr int WN = BN / 4;            // columns per wave
  constexpr int NJ = WN / 16;           // 16-wide n subtiles per wave
  constexpr int MI = 8;                 // 16-high m subtiles per wave (128 rows)
  constexpr int A_BYTES = BM * 128;     // one A panel (256 × 64 bf16)
  constexpr int B_BYTES = BN * 128;
  constexpr int STAGE = A_BYTES + B_BYTES;
  extern __shared__ __attribute__((aligned(1024))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;

  const int tile = hq_xcd_tile(blockIdx.x, gridDim.x);   // then M-major tile order within an XCD
  const int tiles_n = N / BN;
  const int tm = tile / tiles_n, tn = tile % tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  HQ_DASSERT(m0 + BM <= M && n0 + BN <= N && K % BK == 0);

  const uint16_t* Ab = A + (size_t)m0 * lda;
  const uint16_t* Bb = B + (size_t)n0 * ldb;
  const int nt = K / BK;

  // staging split: A panel = 32 pieces of 8 rows (4 per wave); B panel = BN/8 pieces (BN/64 per wave)
  constexpr int A_INSTR = BM / 8 / 8;
  constexpr int B_INSTR = BN / 8 / 8;

  f32x4_t acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  auto stage = [&](int t, int buf) {
    char* base = smem + buf * STAGE;
    stage_panel<A_INSTR>(Ab, lda, wave * (BM / 8), t * BK, base, lane);
    stage_panel<B_INSTR>(Bb, ldb, wave * (BN / 8), t * BK, base + A_BYTES, lane);
  };

  const int fr = lane & 15;           // fragment row within a 16-row subtile
  const int fq = lane >> 4;           // k-slot quarter (8 bf16 each) within a 32-wide k step
  bf16x8_t bf[NJ], af[MI];
  auto read_frags = [&](int t, int ks) {   // R phase: this wave's fragments of k-step ks of tile t
    const char* pa = smem + (t & 1) * STAGE;
    const char* pb = pa + A_BYTES;
#pragma unroll
    for (int j = 0; j < NJ; ++j) bf[j] = frag(pb, wn * WN + j * 16 + fr, ks * 4 + fq);
#pragma unroll
    for (int i = 0; i < MI; ++i) af[i] = frag(pa, wm * 128 + i * 16 + fr, ks * 4 + fq);
  };
  auto mfma_block = [&]() {               // M phase
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] = mfma16(bf[j], af[i], acc[i][j]);
    __builtin_amdgcn_s_setprio(0);
  };
  auto bar = []() { __builtin_amdgcn_s_barrier(); };   // bare: hq_tile::bar()'s compiler fences change this kernel
  auto drain = []() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };

  // Two wave groups (wm = 0: waves 0-3, wm = 1: waves 4-7; a SIMD hosts one wave of each) run the
  // same R/M phase sequence offset by one workgroup barrier, so on every SIMD one wave reads its
  // LDS fragments while the other issues MFMAs.  Group 1 starts with an extra barrier, group 0 ends
  // with one.  Barrier k of group 0 pairs with barrier k of group 1 (one phase later in its program):
  //   RAW: every wave drains its LDS-DMA of tile t before the barrier that precedes the first read of
  //   tile t by either group; WAR: a tile-(t+1) DMA into buffer (t+1)&1 is issued only after the
  //   barrier that follows the other group's last read of tile t-1.
  stage(0, 0);
  drain();
  bar();
  if (__builtin_amdgcn_readfirstlane(wm) == 0) {
    for (int t = 0; t < nt; ++t) {
      if (t + 1 < nt) stage(t + 1, (t + 1) & 1);
      read_frags(t, 0);
      bar();
      mfma_block();
      bar();
      read_frags(t, 1);
      bar();
      mfma_block();
      drain();
      bar();
    }
    bar();
  } else {
    bar();
    for (int t = 0; t < nt; ++t) {
      if (t + 1 < nt) stage(t + 1, (t + 1) & 1);
      read_frags(t, 0);
      bar();
      mfma_block();
      bar();
      read_frags(t, 1);
      drain();
      bar();
      mfma_block();
      bar();
    }
  }

  // ---- epilogue, phase 1: acc (+bias) -> bf16 into this wave's private LDS region [128][WN]
  // (row stride WN*2+16 B keeps the 16-row ds_write_b64 groups at most 2-way and rows 16-B aligned).
  // The last loop barrier guarantees every wave is done reading the A/B panels.
  constexpr int RS = WN * 2 + 16;
  char* wreg = smem + wave * (128 * RS);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int nl = j * 16 + fq * 4;
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (hq_epi_has_bias(EPI)) bv = *reinterpret_cast<const float4*>(bias + n0 + wn * WN + nl);
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      float v[4] = {acc[i][j][0] + bv.x, acc[i][j][1] + bv.y, acc[i][j][2] + bv.z, acc[i][j][3] + bv.w};
      *reinterpret_cast<uint2*>(wreg + (i * 16 + fr) * RS + nl * 2) = hq_pack4(v);
    }
  }
  // ---- phase 2: row-coalesced 16-B pieces (8 columns) -> epilogue math -> 16-B global stores
  constexpr int SEGS = WN / 8;                  // 16-B pieces per row of the wave tile
  constexpr int ROWS_PER_IT = 64 / SEGS;
  const int seg = lane % SEGS, rsub = lane / SEGS;
  const int mb = m0 + wm * 128, nb = n0 + wn * WN + seg * 8;
  const uint16_t* aux_src = hq_epi_col_partials(EPI) ? P : R;
  float csum[8];
  if constexpr (hq_epi_col_partials(EPI)) {
#pragma unroll
    for (int e = 0; e < 8; ++e) csum[e] = 0.f;
  }
#pragma unroll 4
  for (int it = 0; it < 128 / ROWS_PER_IT; ++it) {
    const int row = it * ROWS_PER_IT + rsub;
    uint4 piece = *reinterpret_cast<const uint4*>(wreg + row * RS + seg * 16);
    const size_t goff = (size_t)(mb + row) * ldc + nb;
    hq_epi_piece<EPI>(piece, [&]() -> const uint4& { return *reinterpret_cast<const uint4*>(aux_src + goff); }, goff, dr,
                      key, csum, [&](const uint4& p) { *reinterpret_cast<uint4*>(P + goff) = p; });
    *reinterpret_cast<uint4*>(C + goff) = piece;
  }
  if constexpr (hq_epi_col_partials(EPI)) {
    // column sums: xor-reduce over rsub, then the two M-waves through LDS (after everyone is done with its
    // staging region)
    hq_epi_csum_reduce<SEGS>(csum);
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);  // [2][BN]
    if (rsub == 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) red[wm * BN + wn * WN + seg * 8 + e] = csum[e];
    }
    __syncthreads();
    for (int c = tid; c < BN; c += kThreads) part[(size_t)tm * N + n0 + c] = red[c] + red[BN + c];
  }
}

template <int EPI, int BN>
void launch_v1(const HqNtArgs& a, hipStream_t s) {
  constexpr size_t lds = hq_nt_tile_lds(BN);
  [[maybe_unused]] static const bool once = hq_raise_lds_limit({(const void*)gemm_nt_kernel<EPI, BN>}, lds);
  a.launch(gemm_nt_kernel<EPI, BN>, (a.M / BM) * (a.N / BN), kThreads, lds, s);
}

}  // namespace

void hq_nt_v1_launch(int epi, const HqNtArgs& a, int bn, hipStream_t s) {
  hq_with_epi(epi, [&](auto e) {
    constexpr int EPI = decltype(e)::value;
    if (bn == 256) launch_v1<EPI, 256>(a, s); else launch_v1<EPI, 128>(a, s);
  });
}
