// bf16 NT GEMM, v2 — deep LDS-DMA pipeline (CDNA4 playbook §5 "8-phase" structure, re-derived for this tile).
//
// Same 256×256×64 tile, 8 waves, swizzle and swapped-operand MFMA as v1, but the staging is split into four
// 16 KiB "halves" (128 rows of the A or B panel, 2 LDS-DMA instructions per thread) issued across the K-tile's
// two MFMA phases, so three halves stay in flight across every barrier (counted vmcnt(6), never 0 in the steady
// state) instead of v1's whole-tile issue + vmcnt(0) drain per K-tile.  Quadrants, stage / wait table and hazard
// argument: hq_gemm_tile.h.  Tail K-tiles skip the stages past the end and use the exact smaller vmcnt.
// ABL (production = 8, or 24 for wide N; the rest tools/gemm_lab only): bit0 skip the in-loop LDS-DMA stages, bit1
// skip the in-loop fragment reads, bit2 run both wave groups in lockstep (no stagger barrier), bit3 stage
// with buffer_load … lds (SRD + precomputed per-lane offsets) instead of global_load_lds, bit4
// grouped tile order (8 row panels × all column panels per group).
#include "hq_gemm_epi.h"
#include "hq_gemm_nt.h"
#include "hq_gemm_tile.h"

namespace {

using namespace hq_tile;

template <int EPI, int ABL = 0>
__global__ __launch_bounds__(kThreads, 1) void gemm_nt2_kernel(const uint16_t* __restrict__ A, const uint16_t* __restrict__ B,
                                                               uint16_t* __restrict__ C, const float* __restrict__ bias,
                                                               uint16_t* __restrict__ P, const uint16_t* __restrict__ R,
                                                               float* __restrict__ part, int M, int N, int K, int lda,
                                                               int ldb, int ldc, HqDropArg dr) {
  const uint32_t key = EPI == HQ_EPI_BDR ? dr.kd.get() : 0u;   // EPI_BDR dropout key (device seed word under graphs)
  constexpr int BN = 256;
  constexpr int PANEL = 256 * 128;      // one A or B panel (256 rows × 64 bf16)
  constexpr int STAGE = 2 * PANEL;      // A panel then B panel
  extern __shared__ __attribute__((aligned(1024))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;

  const int nwg = gridDim.x;
  const int bid = blockIdx.x;
  const int tiles_n = N / BN;
  // Half-tile tail (as v3's; production buffer-load form, ungrouped order only): the host launches rt blocks
  // more than there are tiles when the last wave of tiles would be at most half full; blocks F … nwg-1,
  // dispatched last, run the last rt tiles as 2·rt 128-row halves.
  constexpr bool kHalfOK = !hq_epi_col_partials(EPI) && (ABL & 8) != 0 && (ABL & 16) == 0;
  const int ntiles = (M / BM) * tiles_n;
  const int rt = kHalfOK ? nwg - ntiles : 0;
  const int F = nwg - 2 * rt;                    // full-tile blocks (= ntiles - rt)
  const bool half = rt > 0 && bid >= F;
  const int nfull = rt > 0 ? F : nwg;
  const int tile = half ? F + ((bid - F) >> 1) : hq_xcd_tile(bid, nfull);
  int tm = tile / tiles_n, tn = tile % tiles_n;
  if constexpr ((ABL & 16) != 0) {
    constexpr int GM = 8;
    const int tiles_m = M / BM, per = GM * tiles_n;
    const int first = (tile / per) * GM, gsz = min(tiles_m - first, GM), in = tile % per;
    tm = first + in % gsz;
    tn = in / gsz;
  }
  const int m0 = tm * BM + (half ? ((bid - F) & 1) * 128 : 0), n0 = tn * BN;
  HQ_DASSERT(m0 + (half ? 128 : BM) <= M && n0 + BN <= N && K % BK == 0 && K >= 2 * BK);

  const uint16_t* Ab = A + (size_t)m0 * lda;
  const uint16_t* Bb = B + (size_t)n0 * ldb;
  const int nt = K / BK;

  // Staging of one half of K-tile t: buffer_load … lds through SRDs over the block's A / B row panels (a last
  // half tile's panel ends at row M: its unread second 128 rows load as zeros), or (ABL bit 3 clear)
  // global_load_lds, wave w moving rows w·16 .. w·16+15 of the half.  `pro`: the prologue's loads, which are
  // real in the no-load ablation too.
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc((void*)Ab, (short)0, min(BM, M - m0) * lda * 2, kRawBufferWord3);
  __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc((void*)Bb, (short)0, BN * ldb * 2, kRawBufferWord3);
  int voA[2], voB[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row0 = wave * 16 + i * 8;
    voA[i] = lane_src_offset(row0, lane, lda);
    voB[i] = lane_src_offset(row0, lane, ldb);
  }
  // (hq_tile::stage_half's text; through the function this kernel's scalar code around the loads changes)
  auto buf_half = [&](__amdgpu_buffer_rsrc_t rs, const int (&vo)[2], int ld, int half, int t, char* panel) {
    char* dst = panel + (half * 128 + wave_u * 16) * 128;
    const int so = half * 128 * ld * 2 + t * BK * 2;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(dst + i * 8 * 128), 16, vo[i], so, 0, 0);
  };
  auto stA = [&](int half, int t, bool pro = false) {
    if ((ABL & 1) != 0 && !pro) return;
    if constexpr ((ABL & 8) != 0) buf_half(rA, voA, lda, half, t, smem + (t & 1) * STAGE);
    else stage_panel<2>(Ab, lda, half * 128 + wave * 16, t * BK, smem + (t & 1) * STAGE, lane);
  };
  auto stB = [&](int half, int t, bool pro = false) {
    if ((ABL & 1) != 0 && !pro) return;
    if constexpr ((ABL & 8) != 0) buf_half(rB, voB, ldb, half, t, smem + (t & 1) * STAGE + PANEL);
    else stage_panel<2>(Bb, ldb, half * 128 + wave * 16, t * BK, smem + (t & 1) * STAGE + PANEL, lane);
  };

  f32x4_t acc[8][4];   // [mh·4 + i][nh·2 + j]
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  bf16x8_t af[2][4];        // [ks][i] of the current m-half
  bf16x8_t bf0[2][2], bf1[2][2];   // [ks][j] of n-half 0 / 1
  // the no-read ablation reads K-tile 0's fragments only
  auto readA = [&](int t, int mh) {
    if ((ABL & 2) == 0 || t == 0) hq_tile::readA(af, smem + (t & 1) * STAGE, mh, wm, fr, fq);
  };
  auto readB = [&](int t, int nh, bf16x8_t (&bf)[2][2]) {
    if ((ABL & 2) != 0 && t > 0) return;
    const char* pb = smem + (t & 1) * STAGE + PANEL;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[ks][j] = frag(pb, wn * 64 + nh * 32 + j * 16 + fr, ks * 4 + fq);
  };
  auto mma = [&](int mh, int nh, const bf16x8_t (&bf)[2][2]) { hq_tile::mma(acc, af, bf, mh, nh); };

  // prologue: K-tile 0 (A0 B0 B1 A1) and the first three halves of K-tile 1; the wait retires K-tile 0
  stA(0, 0, true); stB(0, 0, true); stB(1, 0, true); stA(1, 0, true);
  stA(0, 1, true); stB(0, 1, true); stB(1, 1, true);
  asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  bar();

  // One K-tile = 2 phases of 32 MFMAs (stage / wait table and hazard argument: hq_gemm_tile.h)
  auto ktile = [&](int t) {
    const bool more1 = t + 1 < nt, more2 = t + 2 < nt;
    // P01 (0,0) (0,1): A1 of K-tile t; younger: the previous P23's three halves (the prologue's at t = 0)
    if (t == 0 || more1) asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    readB(t, 0, bf0);
    readA(t, 0);
    readB(t, 1, bf1);
    if (more1) stA(1, t + 1);
    bar();
    mma(0, 0, bf0);
    mma(0, 1, bf1);
    bar();
    // P23 (1,1) (1,0): K-tile t+1's A0 B0 B1, read by BOTH wave rows in their next P01 (rows of a half come from
    // all 8 waves); younger: this P01's A1.  Both rows wait here, two barriers ahead of the reads.
    if (more1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (!half) readA(t, 1);
    if (more2) { stA(0, t + 2); stB(0, t + 2); stB(1, t + 2); }
    bar();
    if (!half) {
      mma(1, 1, bf1);
      mma(1, 0, bf0);
    }
    bar();
  };
  if (ABL & 4) {
    for (int t = 0; t < nt; ++t) ktile(t);
  } else if (__builtin_amdgcn_readfirstlane(wm) == 0) {
    for (int t = 0; t < nt; ++t) ktile(t);
    bar();
  } else {
    bar();
    for (int t = 0; t < nt; ++t) ktile(t);
  }

  // ---- epilogue (as v1, with the quadrant → tile mapping): acc (+bias) -> bf16 into this wave's
  // private LDS region [128 local rows][64 local cols], local row lr = mh·64 + i·16 + ..,
  // local col lc = nh·32 + j·16 + ..; then row-coalesced 16-B pieces -> epilogue math -> global.
  constexpr int WN = 64;
  constexpr int RS = WN * 2 + 16;
  constexpr int SEGS = WN / 8;                  // 8 pieces of 16 B per local row
  constexpr int ROWS_PER_IT = 64 / SEGS;        // 8
  constexpr int NIT = 128 / ROWS_PER_IT;        // 16 row-coalesced pieces per lane
  constexpr bool kReadsAux = hq_epi_reads_aux(EPI);
  const int seg = lane % SEGS, rsub = lane / SEGS;
  const int gcol = n0 + wn * 64 + seg * 8;   // full 128-B lines per store (see gemm_nt_v3.hip)
  auto grow_of = [&](int it) {
    const int lr = it * ROWS_PER_IT + rsub;
    return m0 + (lr >> 6) * 128 + wm * 64 + (lr & 63);
  };
  char* wreg = smem + wave * (128 * RS);
  // (bias-free epilogues: no "+0" canonicalise adds)
  constexpr bool kBias = hq_epi_has_bias(EPI);
#pragma unroll
  for (int J = 0; J < 4; ++J) {
    const int nh = J >> 1, j = J & 1;
    const int lc = nh * 32 + j * 16 + fq * 4;
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (kBias) bv = *reinterpret_cast<const float4*>(bias + n0 + wn * 64 + nh * 32 + j * 16 + fq * 4);
#pragma unroll
    for (int I = 0; I < 8; ++I) {
      float v[4] = {acc[I][J][0], acc[I][J][1], acc[I][J][2], acc[I][J][3]};
      if constexpr (kBias) { v[0] += bv.x; v[1] += bv.y; v[2] += bv.z; v[3] += bv.w; }  // no "+0" canonicalise adds
      *reinterpret_cast<uint2*>(wreg + (I * 16 + fr) * RS + lc * 2) = hq_pack4(v);
    }
  }
  // The epilogue's second operand (P = stored pre / gelu', R = residual) comes from HBM: issue all 16
  // pieces of this lane at once so ONE load latency is exposed instead of one per few pieces inside the
  // store loop (64 VGPRs; the accumulators are dead now).  Issued after the staging writes: hipcc
  // drains vmcnt(0) before the first LDS write (the main loop's LDS-DMA shares the counter).
  // a half tile has local rows 0..63 only (it < NIT / 2)
  uint4 aux[kReadsAux ? NIT : 1];
  if constexpr (kReadsAux) {
    const uint16_t* src = hq_epi_col_partials(EPI) ? P : R;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {   // a half tile re-reads its rows for the unused pieces (no per-load branch)
      const int itl = half ? (it & (NIT / 2 - 1)) : it;
      aux[it] = *reinterpret_cast<const uint4*>(src + (size_t)grow_of(itl) * ldc + gcol);
    }
  }
  float csum[8];
  if constexpr (hq_epi_col_partials(EPI)) {
#pragma unroll
    for (int e = 0; e < 8; ++e) csum[e] = 0.f;
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    if (half && it >= NIT / 2) continue;
    const int lr = it * ROWS_PER_IT + rsub;
    uint4 piece = *reinterpret_cast<const uint4*>(wreg + lr * RS + seg * 16);
    const size_t goff = (size_t)grow_of(it) * ldc + gcol;
    hq_epi_piece<EPI>(piece, [&]() -> const uint4& { return aux[it]; }, goff, dr, key, csum,
                      [&](const uint4& p) { *reinterpret_cast<uint4*>(P + goff) = p; });
    *reinterpret_cast<uint4*>(C + goff) = piece;
  }
  if constexpr (hq_epi_col_partials(EPI)) {
    hq_epi_csum_reduce<SEGS>(csum);
    __syncthreads();   // red [2][BN] overlaps the staging regions
    float* red = reinterpret_cast<float*>(smem);  // [2][BN], indexed by tile column
    if (rsub == 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) red[wm * BN + (gcol - n0) + e] = csum[e];
    }
    __syncthreads();
    for (int c = tid; c < BN; c += kThreads) part[(size_t)tm * N + n0 + c] = red[c] + red[BN + c];
  }
}

// Production: buffer_load…lds staging (+8-12 % over global_load_lds on the BERT shapes, tools/gemm_lab); grouped
// 8-row-panel tile order only for wide N (+15 % at 8192², neutral at N <= 3072 where an XCD's co-resident tiles
// already share few panels).
template <int EPI>
void launch_v2(const HqNtArgs& a, bool tail, hipStream_t s) {
  constexpr size_t lds = hq_nt_tile_lds(256);
  [[maybe_unused]] static const bool once =
      hq_raise_lds_limit({(const void*)gemm_nt2_kernel<EPI, 8>, (const void*)gemm_nt2_kernel<EPI, 24>}, lds);
  const int grid = (a.M / BM) * (a.N / 256);
  // half-tile tail: rt = grid % CUs more blocks, the last 2·rt of them halves of the last rt tiles
  if (a.N / 256 >= 16) a.launch(gemm_nt2_kernel<EPI, 24>, grid, kThreads, lds, s);
  else a.launch(gemm_nt2_kernel<EPI, 8>, tail ? grid + grid % hq_num_cus() : grid, kThreads, lds, s);
}

}  // namespace

void hq_nt_v2_launch(int epi, const HqNtArgs& a, bool tail, hipStream_t s) {
  hq_with_epi(epi, [&](auto e) { launch_v2<decltype(e)::value>(a, tail, s); });
}
