// bf16 NT GEMM, v3: persistent.
// v2's per-tile fixed cost (WG launch, the prologue's first HBM round trip, the epilogue's drain) is
// ~11k cycles per 256² tile — a third of a K = 768 tile (profiles/s3_prof: the same 464 GFLOP run
// 1.03 PF/s as 4608 K=768 tiles, 1.20 PF/s as 1152 K=3072 tiles).  v3 keeps ONE workgroup per CU
// walking tiles (tile = id, id + grid, …) and runs the LDS-DMA pipeline straight across the tile seam:
// K-tile 0 of the next tile is staged during the last two K-tiles of this one (exactly the loads the
// steady state would issue for t+1 / t+2), so its data lands under the last MFMA phases and the
// epilogue, and the next tile's K-tile-1 A0 / B0 / B1 halves go into the last K-tile's buffer as soon as
// every wave has read it, ahead of the epilogue.
//
// Epilogue LDS: the 128 local rows of each wave are staged in four 32-row rounds through a 4.5 KB region
// per wave — waves 0-2 in the A1 half of the last K-tile's buffer (the next tile stages its K-tile-1 A1 there
// only in its first phase), waves 3-4 past both buffers, waves 5-7 past the bias.  The epilogue's global
// loads/stores (E per lane, EPI-dependent, issued after the next tile's K-tile-1 halves) are counted into
// the first K-tile's vmcnt waits.  Raw barriers only (a __syncthreads fence would drain
// the in-flight DMA).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "hq_gemm_epi.h"
#include "hq_gemm_nt.h"
#include "hq_gemm_tile.h"

namespace {

using namespace hq_tile;

// HQ_EPI_DIAG (lab builds only, never in the production library): bit 0 = the persistent kernel's epilogue issues no
// global stores (data kept live), bit 1 = GELUD skips the GELU math — isolates store cost from VALU cost.
#ifndef HQ_EPI_DIAG
#define HQ_EPI_DIAG 0
#endif
// Cache policy of the persistent kernel's epilogue stores (gfx950 CPol bits: 1 = sc0, 2 = nt, 16 = sc1).  NTS
// kernels store with nt | sc1 — streamed past the caches: at K = 768 the output is a third of the kernel's work in
// bytes and its default-policy write-back holds the next tiles' LDS-DMA operand loads up (the stores retire, in
// vmcnt order, ahead of them); nt | sc1 made the K = 768 NONE / BIAS / GELU / GELUD GEMMs 6-11 % faster on one box
// (profiles/r5_epi_diag/aux*.log), while the K = 2304 / 3072 shapes and the epilogues that load an operand (DMUL /
// RESID) lost 0-3 %.  HQ_EPI_STORE_AUX (lab builds) forces the bits for every variant.
#ifndef HQ_EPI_STORE_AUX
#define HQ_EPI_STORE_AUX 0
#endif
template <int EPI>
struct NT3Epi {
  static constexpr int kStores = (HQ_EPI_DIAG & 1) ? 0 : 16 * (1 + (hq_epi_writes_p(EPI) ? 1 : 0));
  static constexpr int kLoads = hq_epi_reads_aux(EPI) ? 16 : 0;
  static constexpr int E = kStores + kLoads;   // vm ops per lane (the part store of waves 0-3 is not counted: a
};                                             // smaller count only waits longer)

// DYN: the per-XCD ticket schedule is compiled in (a launch with sched == nullptr runs the static one either
// way).  The static-only build (DYN = false, the single-GPU default) has no ticket atomic, whose pending return
// makes hipcc drain vmcnt(0) — the next tile's in-flight K-tile-0 DMA — at every tile's epilogue.
template <int EPI, bool DYN, bool NTS>
__global__ __launch_bounds__(kThreads, 1) void gemm_nt3_kernel(const uint16_t* __restrict__ A, const uint16_t* __restrict__ B,
                                                               uint16_t* __restrict__ C, const float* __restrict__ bias,
                                                               uint16_t* __restrict__ P, const uint16_t* __restrict__ R,
                                                               float* __restrict__ part, int M, int N, int K, int lda,
                                                               int ldb, int ldc, int stagger, unsigned* __restrict__ sched,
                                                               HqDropArg dr) {
  const uint32_t key = EPI == HQ_EPI_BDR ? dr.kd.get() : 0u;   // EPI_BDR dropout key (device seed word under graphs)
  constexpr int BN = 256;
  constexpr int PANEL = 256 * 128;
  constexpr int STAGE = 2 * PANEL;
  constexpr int WN = 64;
  constexpr int RS = WN * 2 + 16;
  constexpr int REGION = 64 * RS;            // one wave's 64-row staging round (9216 B)
  constexpr int SPARE = 2 * STAGE;           // past both stage buffers: wave 7's region, then csum scratch
  constexpr int E = NT3Epi<EPI>::E;
  constexpr int TICKET = SPARE + REGION + 2 * BN * 4;   // LDS word: the tile after `next` (dynamic schedule)
  constexpr int BIASL = TICKET + 16;                    // the unit's 256 fp32 bias values (1 KiB, LDS-DMA by wave 0)
  // epilogue staging: 32-row rounds, QREG bytes per wave — waves 0-2 in the A1 half of the last K-tile's
  // buffer, 3-4 in SPARE, 5-7 past the bias — so that the buffer's other three halves take the next tile's
  // K-tile 1 BEFORE the epilogue's stores (vmcnt retires in issue order: K-tile 1 issued after the stores
  // could not be waited for before they drained, which the first K-tile's counted waits then did)
  constexpr int QREG = 32 * RS;
  constexpr int TAIL = BIASL + 1024;
  static_assert(3 * QREG <= PANEL / 2 && 2 * QREG <= REGION && TAIL + 3 * QREG <= 160 * 1024, "LDS plan");
  constexpr bool kBias = hq_epi_has_bias(EPI);
  const bool ht_on = (stagger >> 16) & 1;   // kHqNtHalfTail
  const bool quarter_on = (stagger >> 17) & 1;
  stagger &= 0xFF;
  extern __shared__ __attribute__((aligned(1024))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);

  const int nwg = gridDim.x, bid = blockIdx.x, xcd = bid & 7;
  const int id = hq_xcd_tile(bid, nwg);
  const int tiles_n = N / BN, ntiles = (M / BM) * tiles_n;
  // The epilogue's bias comes through LDS: wave 0 stages a unit's 256 values with one LDS-DMA instruction at the
  // unit's start (retired by the K-loop's counted waits, made visible by its barriers), and the epilogue reads
  // them with inline-asm ds_reads — a global load there would wait (vmcnt, in issue order) for the next tile's
  // K-tile-0 DMA still in flight, and a builtin LDS read makes hipcc drain vmcnt(0) for the same reason.
  auto stage_bias = [&](int n0u) {
    if constexpr (kBias) {
      if (__builtin_amdgcn_readfirstlane(wave) == 0) {
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)bias, (short)0, N * 4, kRawBufferWord3);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (lds_void*)(smem + BIASL), 16, lane * 16, n0u * 4, 0, 0);
      }
    }
  };

  const int nt = K / BK;
  HQ_DASSERT(K % BK == 0 && nt >= 2 && N % BN == 0 && M % BM == 0);
  // Half-tile tail: when the last wave of tiles is at most half full (rtail = ntiles % nwg tiles on nwg
  // workgroups), its rtail tiles run as 2·rtail 128-row "half tiles", one per workgroup, so that wave costs about
  // half a tile's time instead of a whole one (at B = 256 every N = 768 GEMM has 4.5 waves of tiles).  Work
  // units: 0 … F-1 the full tiles, F … F+2·rtail-1 the halves (unit F + 2h + e = rows e·128 … of tile F + h).  A
  // half tile keeps the full tile's load / barrier / wait sequence (its second 128 A rows are staged and
  // never read) and skips the m-half-1 MFMA phases, fragment reads and epilogue round.  Column partials
  // (DGELU / DMUL) are per 256-row block, so those epilogues never split.
  constexpr bool kHalfOK = !hq_epi_col_partials(EPI);
  const int rtail = ntiles % nwg;
  const bool halftail = kHalfOK && ht_on && rtail > 0 && 2 * rtail <= nwg;
  const int F = halftail ? ntiles - rtail : ntiles;
  const int nunits = halftail ? F + 2 * rtail : ntiles;
  auto unit_m0 = [&](int u) {
    return u < F ? (u / tiles_n) * BM : ((F + ((u - F) >> 1)) / tiles_n) * BM + ((u - F) & 1) * 128;
  };
  auto unit_n0 = [&](int u) { return (u < F ? u : F + ((u - F) >> 1)) % tiles_n * BN; };

  int voA[2], voB[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row0 = wave * 16 + i * 8;
    voA[i] = lane_src_offset(row0, lane, lda);
    voB[i] = lane_src_offset(row0, lane, ldb);
  }
  // buffer descriptors over a unit's A row panel / B column panel (a last half tile's panel ends at row M:
  // its unread second 128 rows load as zeros)
  auto rsrc_a = [&](int u) {
    const int m0 = unit_m0(u);
    return __builtin_amdgcn_make_buffer_rsrc((void*)(A + (size_t)m0 * lda), (short)0, min(BM, M - m0) * lda * 2,
                                             kRawBufferWord3);
  };
  auto rsrc_b = [&](int u) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)(B + (size_t)unit_n0(u) * ldb), (short)0, BN * ldb * 2, kRawBufferWord3);
  };
  // one 16 KiB half (128 rows × 64 bf16) of K-tile `kt` into LDS buffer `buf`
  auto stA = [&](__amdgpu_buffer_rsrc_t rs, int half, int kt, int buf) {
    stage_half<2>(rs, voA, lda, half, kt, smem + buf * STAGE, wave_u);
  };
  auto stB = [&](__amdgpu_buffer_rsrc_t rs, int half, int kt, int buf) {
    stage_half<2>(rs, voB, ldb, half, kt, smem + buf * STAGE + PANEL, wave_u);
  };

  f32x4_t acc[8][4];
  const int fr = lane & 15, fq = lane >> 4;
  bf16x8_t af[2][4];
  bf16x8_t bf0[2][2], bf1[2][2];
  auto readA = [&](int buf, int mh) { hq_tile::readA(af, smem + buf * STAGE, mh, wm, fr, fq); };
  auto readB = [&](int buf, int nh, bf16x8_t (&bf)[2][2]) {
    const char* pb = smem + buf * STAGE + PANEL;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[ks][j] = frag(pb, wn * 64 + nh * 32 + j * 16 + fr, ks * 4 + fq);
  };
  auto mma = [&](int mh, int nh, const bf16x8_t (&bf)[2][2]) { hq_tile::mma(acc, af, bf, mh, nh); };

  // Tile schedule.  Static: tile id, id + nwg, id + 2·nwg, …  — the blocks of one XCD (x = bid & 7, the
  // cnt_x workgroups with ids base_x … base_x + cnt_x - 1) walk, round after round, the same contiguous
  // run of cnt_x tiles, so their A row panels stay in that XCD's L2.  Dynamic (sched != null) keeps that
  // per-XCD sequence, tile(s) = (s / cnt_x)·nwg + base_x + s % cnt_x, but hands out its entries s ≥ 2·cnt_x
  // by tickets from the XCD's own counter (sched[32·x]); the first two (s = j, cnt_x + j) stay static, as the
  // pipeline stages the next tile's K-tile 0 during this tile's last K-tiles, so `next` must be known when
  // this tile starts.  A workgroup dispatched late — its CU held by another stream's kernel, e.g. the RCCL
  // all-reduce overlapped with the backward — then delays only its first two tiles instead of its whole
  // 1/nwg share (tools/gemm_contention_bench.py).  The ticket is drawn by thread 0 early in the tile
  // (a per-lane address keeps hipcc's atomic optimizer — whose readfirstlane would wait for the return on
  // the spot — out of it) and published through LDS after the K-loop, where hipcc drains vmcnt anyway.
  // Every workgroup bumps sched[256] on exit; the last one zeroes the counters for the next launch on this
  // stream (stream order: the next launch starts after this one has drained, graph replays included).
  int tile = id;                // a work unit (see the half-tile tail above)
  HQ_DASSERT(tile < nunits);     // the host launches min(tiles, CUs) workgroups, so every one has a tile
  if (tile >= nunits) return;   // (unreachable; an early exit would skip the exit count that re-zeroes sched)
  int next = tile + nwg;
  const int cnt_x = (nwg >> 3) + (xcd < (nwg & 7) ? 1 : 0), base_x = id - (bid >> 3);
  if constexpr (!DYN) sched = nullptr;
  unsigned* tix = sched ? sched + 32 * xcd : nullptr;
  // Phase offset for half of each XCD's workgroups (stagger × 8128 cycles): the tile seams of all CUs
  // otherwise coincide, and every epilogue's stores / aux loads hit HBM in one chip-wide burst that the
  // next K-tile's counted wait (vmcnt counts stores too) then stalls on.
  // bit 17 of the flag word: four groups (offsets 0, 1, 2, 3 × stagger) instead of two (0, stagger)
  const int sgroup = quarter_on ? ((bid >> 3) & 3) : ((bid >> 3) & 1);
  for (int i = 0; i < stagger * sgroup; ++i) __builtin_amdgcn_s_sleep(127);
  __amdgpu_buffer_rsrc_t ca = rsrc_a(tile), cb = rsrc_b(tile);
  int p0 = 0;                   // LDS buffer of this tile's K-tile 0
  // prologue of the first tile: K-tile 0 (A0 B0 B1 A1) and K-tile 1's A0 B0 B1 (its A1 is staged in K-tile 0)
  stage_bias(unit_n0(tile));   // oldest op of wave 0: retired by the wait below
  stA(ca, 0, 0, 0); stB(cb, 0, 0, 0); stB(cb, 1, 0, 0); stA(ca, 1, 0, 0);
  stA(ca, 0, 1, 1); stB(cb, 0, 1, 1); stB(cb, 1, 1, 1);
  asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  bar();
  bool first = true;
  bool prev_half = false;       // the previous unit was a half tile: its epilogue issued E / 2 vm ops

  for (;;) {
    const bool last = next >= nunits;
    const bool half = __builtin_amdgcn_readfirstlane(tile >= F ? 1 : 0) != 0;
    unsigned ticket = 0;
    const bool draw = DYN && sched && !last;
    // drawn in phase P1 of K-tile 0, after that phase's stage: the counted vmcnt(6) of K-tile 1's P1 (6 newer
    // loads by then) retires it about a K-tile later, so its round trip never stalls a wait (issued at the
    // tile top it was the OLDEST op under K-tile 0's first wait and cost ~1-3 % per GEMM)
    auto draw_ticket = [&]() {
      if (tid == 0) {
        unsigned zero;
        asm volatile("v_mov_b32 %0, 0" : "=v"(zero));   // opaque per-lane offset (see above)
        ticket = __hip_atomic_fetch_add(tix + zero, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    };
    const __amdgpu_buffer_rsrc_t na = rsrc_a(last ? tile : next), nb = rsrc_b(last ? tile : next);
    const int m0 = unit_m0(tile), n0 = unit_n0(tile);
    const int tm = m0 / BM;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // One K-tile = 2 phases of 32 MFMAs per wave (stage / wait table and hazard argument: hq_gemm_tile.h).  Past
    // this tile's end the stages come from the next tile's K-tile 0 (t+1 == nt, t+2 == nt); its K-tile-1 A0 B0 B1
    // (t+2 == nt+1) go into buffer bl right after the last K-tile.
    auto ktile = [&](int t) {
      const bool more1 = t + 1 < nt || !last;                    // P01 stages A1 of K-tile t+1
      const bool more2 = t + 2 < nt || (t + 2 == nt && !last);    // P23 stages K-tile t+2 (A0 B0 B1)
      const bool prev2 = t + 1 < nt || (t + 1 == nt && !last);    // P23 of K-tile t-1 staged K-tile t+1
      const int b0 = (p0 + t) & 1, b1 = b0 ^ 1;
      const bool x1 = t + 1 >= nt, x2 = t + 2 >= nt;        // the "ahead" halves belong to the next tile
      const __amdgpu_buffer_rsrc_t a1 = x1 ? na : ca;
      const __amdgpu_buffer_rsrc_t a2 = x2 ? na : ca, b2r = x2 ? nb : cb;
      const int k1 = x1 ? t + 1 - nt : t + 1, k2 = x2 ? t + 2 - nt : t + 2;
      // P01 wait (at t = 0 of a following unit the previous epilogue's E vm ops, E / 2 after a half tile, are younger)
      // HQ_EPI_DIAG bit 3 (timing lab only, results WRONG): no vmcnt wait in K-tiles 1-7 of a following unit, i.e.
      // what the mainloop would cost if the previous epilogue's stores never held up the DMA waits
      // bit 4: no vmcnt wait in ANY K-tile of a following unit (pure issue timing, results wrong)
      const bool relax = ((HQ_EPI_DIAG & 8) && !first && t >= 1 && t < 8) || ((HQ_EPI_DIAG & 16) && !first);
      if (relax) {
      } else if (t == 0 && !first) {
        if (prev_half) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(6 + E / 2) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" :: "n"(6 + E) : "memory");
      } else if (t == 0 || prev2) {
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      readB(b0, 0, bf0);
      readA(b0, 0);
      readB(b0, 1, bf1);
      if (more1) stA(a1, 1, k1, b1);
      if (t == 0 && draw) draw_ticket();
      bar();
      mma(0, 0, bf0);
      mma(0, 1, bf1);
      bar();
      // P23 wait, both wave rows
      if (relax) {
      } else if (t == 0 && !first) {
        if (prev_half) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 + E / 2) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 + E) : "memory");
      } else if (more1) {
        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      if (!half) readA(b0, 1);
      if (more2) { stA(a2, 0, k2, b0); stB(b2r, 0, k2, b0); stB(b2r, 1, k2, b0); }
      bar();
      if (!half) {
        mma(1, 1, bf1);
        mma(1, 0, bf0);
      }
      bar();
    };
    if (__builtin_amdgcn_readfirstlane(wm) == 0) {
      for (int t = 0; t < nt; ++t) ktile(t);
      bar();
    } else {
      bar();
      for (int t = 0; t < nt; ++t) ktile(t);
    }
    // every wave has passed its last MFMA phase: the buffer of the last K-tile is free
    if (draw && tid == 0)
      *reinterpret_cast<unsigned*>(smem + TICKET) = 2u * (unsigned)cnt_x + ticket;   // sequence index s
    const int bl = (p0 + nt - 1) & 1;
    char* wreg = wave < 3 ? smem + bl * STAGE + PANEL / 2 + wave * QREG
                          : (wave < 5 ? smem + SPARE + (wave - 3) * QREG : smem + TAIL + (wave - 5) * QREG);
    // every wave is past its last read of buffer bl: the next tile's K-tile-1 A0 / B0 / B1 halves go there now,
    // ahead of the epilogue's loads and stores (its A1 half holds waves 0-2's staging; P01 of K-tile 0 stages it)
    if (!last) { stA(na, 0, 1, bl); stB(nb, 0, 1, bl); stB(nb, 1, 1, bl); }

    // ---- epilogue (v2's math), 32 local rows per round (4 rounds, 2 in a half tile).  Ordered so that no round
    // waits for an earlier round's stores (vmcnt counts loads and stores in issue order): the bias and ALL the
    // epilogue operands (aux: 16 pieces per lane, 64 VGPRs — the fragment registers are dead) are loaded before
    // the first store, and the staging writes are inline-asm ds_writes, which hipcc does not fence with vmcnt(0)
    // as it does a builtin LDS store while LDS-DMA may be in flight.  Nothing targets a wave's staging region by
    // DMA during the epilogue, and LDS executes a wave's ds operations in order, so a round's writes cannot
    // overtake the previous round's reads.
    constexpr int SEGS = WN / 8, ROWS_PER_IT = 64 / SEGS;
    constexpr bool kReadsAux = hq_epi_reads_aux(EPI);
    const int seg = lane % SEGS, rsub = lane / SEGS;
    // wave column wn owns the 64 contiguous tile columns wn·64 … +63 (B fragments nh·32 + j·16 inside it), so each
    // store instruction writes 8 rows × one full 128-B line — the earlier wn·32 + {0, 128} map wrote two 64-B half
    // lines per row, each line split between two waves: −2…−3 % on every K = 768 GEMM, +1.45 % step
    // (profiles/r6_lines)
    const int gcol = n0 + wn * 64 + seg * 8;
    const uint32_t wreg_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)wreg;
    // round q: rows (q >> 1)·128 + wm·64 + (q & 1)·32 + it·8 + rsub of the tile (it: 0..3 within the round)
    auto goff_of = [&](int q, int it) {
      return (size_t)(m0 + (q >> 1) * 128 + wm * 64 + (q & 1) * 32 + it * ROWS_PER_IT + rsub) * ldc + gcol;
    };
    // epilogue global traffic through buffer descriptors over the unit's rows: ONE per-lane offset register
    // (row rsub of the wave's 64-row block, column gcol) and a wave-uniform scalar offset per piece, instead
    // of a 64-bit address per piece (16 pieces × 2 VGPRs spilled once both rounds' operands are prefetched)
    const int rows_u = half ? 128 : BM;
    auto rsrc_of = [&](const uint16_t* base) {
      return __builtin_amdgcn_make_buffer_rsrc((void*)(base + (size_t)m0 * ldc), (short)0, rows_u * ldc * 2, kRawBufferWord3);
    };
    const int vo_lane = ((wm * 64 + rsub) * ldc + gcol) * 2;
    auto so_of = [&](int q, int it) { return ((q >> 1) * 128 + (q & 1) * 32 + it * ROWS_PER_IT) * ldc * 2; };
    auto bload = [&](__amdgpu_buffer_rsrc_t r, int rnd, int it) {
#if HQ_EPI_DIAG & 64
      // bit 6 (timing lab only, results WRONG): every operand load reads the tile's first 8 rows (L2-resident):
      // what the epilogue would cost if the operand never came from HBM
      const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, vo_lane & 0xFFFF, 0, 0);
#else
      const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, vo_lane, so_of(rnd, it), 0);
#endif
      return make_uint4(v.x, v.y, v.z, v.w);
    };
    // STORE-DATA HOLD.  A dwordx4 store can read its data VGPRs well after it issued when the wave has a
    // queue of stores (and LDS-DMA) in flight: measured on MI355X, the GELU epilogue's P store (its data
    // overwritten by the GELU math 5 instructions later — hipcc pads 1-2 wait states) wrote the NEW value into
    // dword 0 of 16-lane groups 1 and 3 (~3e-5 of the elements, varying run to run).  So every store's data
    // stays live (an empty asm use) until the NEXT piece's stores have issued, and each round ends with a
    // 64-wait-state pad that holds the last piece (and, for BIAS's back-to-back stores, every piece).
    auto bstore = [&](__amdgpu_buffer_rsrc_t r, int rnd, int it, const uint4& d) {
      const u32x4_t v = {d.x, d.y, d.z, d.w};
#if HQ_EPI_DIAG & 1
      asm volatile("" :: "v"(v));
#elif HQ_EPI_DIAG & 32
      // bit 5: every store goes to the tile's first 8 rows (L2-resident): issue cost without the HBM write traffic
      __builtin_amdgcn_raw_buffer_store_b128(v, r, vo_lane & 0xFFFF, 0, 0);
#else
      __builtin_amdgcn_raw_buffer_store_b128(v, r, vo_lane, so_of(rnd, it), HQ_EPI_STORE_AUX | (NTS ? 18 : 0));
#endif
      return v;
    };
    float csum[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) csum[e] = 0.f;
    // NR = 2 row halves (full tile) or 1 (half tile), a compile-time count: with a runtime `half` test hipcc
    // sinks the later rounds' operand loads into the branch, i.e. behind the first round's stores
    auto epilogue = [&](auto nr_c) {
      constexpr int NR = decltype(nr_c)::value;
      // BDR keeps per-round operand loads (both rounds' 64 VGPRs spill beside its dropout hash)
      constexpr bool kAll = kReadsAux && EPI != HQ_EPI_BDR;
      f32x4_t bvs[4] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f},
                        f32x4_t{0.f, 0.f, 0.f, 0.f}};
      if constexpr (kBias) {   // J = 0..3 at byte offsets 0, 64, 128, 192 (cols +0, +16, +32, +48); one statement
        const uint32_t bias_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)(smem + BIASL);
        asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:64\n\tds_read_b128 %2, %4 offset:128\n\t"
                     "ds_read_b128 %3, %4 offset:192\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(bvs[0]), "=&v"(bvs[1]), "=&v"(bvs[2]), "=&v"(bvs[3])
                     : "v"(bias_lds + (uint32_t)((wn * 64 + fq * 4) * 4))
                     : "memory");
      }
      const __amdgpu_buffer_rsrc_t rC = rsrc_of(C);
      const __amdgpu_buffer_rsrc_t rP = rsrc_of(P ? P : C);
      const __amdgpu_buffer_rsrc_t rA = hq_epi_col_partials(EPI) ? rP : rsrc_of(R);   // aux source
      constexpr int NQ = 2 * NR;   // 32-row rounds
      uint4 aux[kReadsAux ? (kAll ? 8 * NR : 4) : 1];
      // per round: stage (inline-asm ds_writes: no vmcnt fence), read its 4 pieces back, math, stores; the
      // second row half's operands are loaded after the first round's staging, still before its first store
      uint4 pieces[NQ][4];
      // acc (+bias) → bf16 pairs for every round up front: the 128 accumulator VGPRs die here (64 hold the packed
      // tile), which is what lets both rounds' operands and a round of pieces stay in registers without spilling
      u32x2_t pk[NR][16];
#pragma unroll
      for (int rnd = 0; rnd < NR; ++rnd)
#pragma unroll
        for (int J = 0; J < 4; ++J) {
          const f32x4_t bv = bvs[J];
#pragma unroll
          for (int I = 0; I < 4; ++I) {
            const f32x4_t& a = acc[rnd * 4 + I][J];
            float v[4] = {a[0], a[1], a[2], a[3]};
            if constexpr (kBias) { v[0] += bv[0]; v[1] += bv[1]; v[2] += bv[2]; v[3] += bv[3]; }
            const uint2 q = hq_pack4(v);
            pk[rnd][J * 4 + I] = u32x2_t{q.x, q.y};
          }
        }
      __builtin_amdgcn_sched_barrier(0);   // packed now, not sunk to the staging (the fp32 accumulators die)
      if constexpr (kAll) {   // the first row half's operands now (their latency hides under the staging) ...
#pragma unroll
        for (int it = 0; it < 8; ++it) aux[it] = bload(rA, it >> 2, it & 3);
      }
      auto stage_round = [&](int q) {   // rows (q & 1)·32 … +31 of row half q >> 1: 16-row blocks I = 2·(q & 1) + i
        const int rnd = q >> 1, sub = q & 1;
#pragma unroll
        for (int J = 0; J < 4; ++J) {
          const int nh = J >> 1, j = J & 1;
          const int lc = nh * 32 + j * 16 + fq * 4;
#pragma unroll
          for (int i = 0; i < 2; ++i)
            asm volatile("ds_write_b64 %0, %1" :: "v"(wreg_lds + (uint32_t)((i * 16 + fr) * RS + lc * 2)),
                         "v"(pk[rnd][J * 4 + 2 * sub + i]) : "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if constexpr (!kReadsAux) {
          // inline asm: a builtin LDS read would make hipcc drain vmcnt(0), i.e. wait for the next tile's
          // K-tile DMA (epilogues with operand loads wait for those, which are younger, anyway).  The reads and
          // their lgkmcnt wait are ONE asm statement: the outputs are defined only when it completes (with
          // separate statements hipcc may copy an output register before the data has returned).
          static_assert(ROWS_PER_IT * RS == 1152, "ds_read offsets below");
          u32x4_t v0, v1, v2, v3;
          asm volatile(
              "ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:1152\n\tds_read_b128 %2, %4 offset:2304\n\t"
              "ds_read_b128 %3, %4 offset:3456\n\ts_waitcnt lgkmcnt(0)"
              : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3)
              : "v"(wreg_lds + (uint32_t)(rsub * RS + seg * 16))
              : "memory");
          const u32x4_t vv[4] = {v0, v1, v2, v3};
#pragma unroll
          for (int it = 0; it < 4; ++it) pieces[q][it] = make_uint4(vv[it].x, vv[it].y, vv[it].z, vv[it].w);
        } else {
#pragma unroll
          for (int it = 0; it < 4; ++it)
            pieces[q][it] = *reinterpret_cast<const uint4*>(wreg + (it * ROWS_PER_IT + rsub) * RS + seg * 16);
        }
      };
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        if (q > 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the previous round's piece reads returned
        stage_round(q);
        if constexpr (kAll && NR > 1) {
          if (q == 0) {   // the second row half's operands: after the first staging, before its stores
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int it = 0; it < 8; ++it) aux[8 + it] = bload(rA, 2 + (it >> 2), it & 3);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        if constexpr (kReadsAux && !kAll) {
#pragma unroll
          for (int it = 0; it < 4; ++it) aux[it] = bload(rA, q, it);
        }
        constexpr bool kTwo = hq_epi_writes_p(EPI);   // P and C stores per piece
        u32x4_t holdP = {0u, 0u, 0u, 0u}, holdC = holdP;                    // the previous piece's store data
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          uint4 piece = pieces[q][it];
          const size_t goff = goff_of(q, it);
          u32x4_t sP = holdP;
          hq_epi_piece<EPI, (HQ_EPI_DIAG & 2) != 0>(piece, [&] { return aux[kAll ? q * 4 + it : it]; }, goff, dr, key, csum,
                                                    [&](const uint4& p) { sP = bstore(rP, q, it, p); });
          const u32x4_t sC = bstore(rC, q, it, piece);
          if (it > 0) {
            if constexpr (kTwo) asm volatile("" :: "v"(holdP), "v"(holdC));
            else asm volatile("" :: "v"(holdC));
          }
          holdP = sP;
          holdC = sC;
          // column-partial epilogues: one piece at a time (hipcc otherwise computes every piece's products
          // ahead of the serial csum chain and spills them)
          if constexpr (hq_epi_col_partials(EPI)) __builtin_amdgcn_sched_barrier(0);
        }
        // round end: 64 wait states with the last stores' data held (BIAS stores back to back: all 4 pieces)
#define HQ_PAD64 "s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15"
        if constexpr (EPI == HQ_EPI_BIAS) {
          auto u = [&](int i) { const uint4& w = pieces[q][i]; return u32x4_t{w.x, w.y, w.z, w.w}; };
          asm volatile(HQ_PAD64 :: "v"(u(0)), "v"(u(1)), "v"(u(2)), "v"(u(3)));
        } else if constexpr (kTwo) {
          asm volatile(HQ_PAD64 :: "v"(holdP), "v"(holdC));
        } else {
          asm volatile(HQ_PAD64 :: "v"(holdC));
        }
#undef HQ_PAD64
      }
    };
    if constexpr (!kHalfOK) epilogue(std::integral_constant<int, 2>{});   // column partials: never a half tile
    else if (half) epilogue(std::integral_constant<int, 1>{});
    else epilogue(std::integral_constant<int, 2>{});
    if constexpr (hq_epi_col_partials(EPI)) {
      hq_epi_csum_reduce<SEGS>(csum);
      float* red = reinterpret_cast<float*>(smem + SPARE + REGION);  // [2][BN], by tile column
      if (rsub == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) red[wm * BN + (gcol - n0) + e] = csum[e];
      }
      bar();
      for (int c = tid; c < BN; c += kThreads) part[(size_t)tm * N + n0 + c] = red[c] + red[BN + c];
    }
    if (last) break;
    // every wave has read the bias (and its staging rounds): stage the next unit's bias (an extra, younger op of
    // wave 0 only: its counted waits wait longer)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    bar();
    stage_bias(unit_n0(next));
    int after = next + nwg;
    if (sched) {
      const unsigned sx = *reinterpret_cast<const unsigned*>(smem + TICKET);
      const long t = (long)(sx / (unsigned)cnt_x) * nwg + base_x + (long)(sx % (unsigned)cnt_x);
      after = t < nunits ? (int)t : nunits;
    }
    prev_half = half;
    tile = next;
    next = __builtin_amdgcn_readfirstlane(after);
    ca = na;
    cb = nb;
    p0 = (p0 + nt) & 1;
    first = false;
  }
  if (sched && tid == 0) {
    if (__hip_atomic_fetch_add(sched + 256, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)nwg - 1) {
      for (int x = 0; x < 8; ++x) __hip_atomic_store(sched + 32 * x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(sched + 256, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// v3 flag word (hq_gemm_set_stagger, tests / lab tools only): start offset of odd workgroups per XCD in units of
// s_sleep(127) (bits 0-7, 0 in production); bit 16 (kHqNtHalfTail): a last, at most half-full wave of tiles runs
// as 128-row half tiles (on); bit 17: four start-offset groups instead of two
int g_gemm_stagger = kHqNtHalfTail;

// epilogue store cache policy of the persistent kernel (see HQ_EPI_STORE_AUX): 1 = streamed stores for the
// operand-free epilogues at K <= 768 (production), 0 = default policy everywhere, 2 = streamed at any K (A/B only)
int g_store_policy = 1;

// default static: uncontended the dynamic schedule costs ~0.9 % of the step (profiles/r2_sched); GradReducer
// switches it on when an all-reduce overlaps the backward (world > 1); HQ_GEMM_SCHED overrides either way
int g_gemm_sched = [] {
  const char* e = getenv("HQ_GEMM_SCHED");
  return e ? atoi(e) : 0;
}();

// Per (device, stream) slot of the v3 ticket schedule: 8 per-XCD ticket counters and the exit counter,
// each on its own 128-B line (words 32·x, 256), carved from one 64-slot block per device that is
// allocated and zeroed on the first use (an eager call: no allocation inside a graph capture once the
// step has run once).  Stream order serialises the launches that share a slot.
constexpr size_t kSchedWords = 9 * 32;
struct SchedPool { unsigned* base = nullptr; std::vector<hipStream_t> streams; };
std::mutex g_sched_mu;

// the current device's pool, allocated and zeroed on first use (caller holds g_sched_mu)
SchedPool* sched_pool_locked() {
  static std::vector<SchedPool> pools;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if ((int)pools.size() <= dev) pools.resize(dev + 1);
  SchedPool& p = pools[dev];
  if (!p.base) {
    void* q = nullptr;
    if (hipMalloc(&q, 64 * kSchedWords * sizeof(unsigned)) != hipSuccess ||
        hipMemset(q, 0, 64 * kSchedWords * sizeof(unsigned)) != hipSuccess) {
      fprintf(stderr, "nt3 tile schedule: slot allocation failed, static schedule\n");
      g_gemm_sched = 0;
      return nullptr;
    }
    p.base = static_cast<unsigned*>(q);
  }
  return &p;
}

unsigned* nt3_sched_slot(hipStream_t s) {
  std::lock_guard<std::mutex> lock(g_sched_mu);
  SchedPool* p = sched_pool_locked();
  if (!p) return nullptr;
  for (size_t i = 0; i < p->streams.size(); ++i)
    if (p->streams[i] == s) return p->base + kSchedWords * i;
  if (p->streams.size() >= 64) return nullptr;   // more streams than slots: static schedule on the rest
  p->streams.push_back(s);
  return p->base + kSchedWords * (p->streams.size() - 1);
}

template <int EPI>
void launch_v3(const HqNtArgs& a, hipStream_t s) {
  constexpr size_t lds = 2 * 2 * 256 * 128 + 64 * 144 + 2 * 256 * 4 + 16 + 1024 + 3 * 32 * 144;
  [[maybe_unused]] static const bool once = hq_raise_lds_limit(
      {(const void*)gemm_nt3_kernel<EPI, false, false>, (const void*)gemm_nt3_kernel<EPI, true, false>,
       (const void*)gemm_nt3_kernel<EPI, false, true>, (const void*)gemm_nt3_kernel<EPI, true, true>}, lds);
  const int grid = (a.M / BM) * (a.N / 256), nwg = std::min(grid, hq_num_cus());
  unsigned* sched = (g_gemm_sched && grid > 2 * nwg) ? nt3_sched_slot(s) : nullptr;
  // streamed (nt | sc1) epilogue stores: epilogues without an operand load, K <= 768 (g_store_policy 1), or at any K
  // (2, A/B only), or never (0)
  const bool nts = !hq_epi_reads_aux(EPI) && (g_store_policy == 2 || (g_store_policy == 1 && a.K <= 768));
  auto go = [&](auto kern) { a.launch(kern, nwg, kThreads, lds, s, g_gemm_stagger, sched); };
  if (sched) {
    if (nts) go(gemm_nt3_kernel<EPI, true, true>); else go(gemm_nt3_kernel<EPI, true, false>);
  } else {
    if (nts) go(gemm_nt3_kernel<EPI, false, true>); else go(gemm_nt3_kernel<EPI, false, false>);
  }
}

}  // namespace

void hq_nt_v3_launch(int epi, const HqNtArgs& a, hipStream_t s) {
  hq_with_epi(epi, [&](auto e) { launch_v3<decltype(e)::value>(a, s); });
}
int hq_nt_v3_flags() { return g_gemm_stagger; }

void hq_gemm_set_store_policy(int v) { g_store_policy = v; }
void hq_gemm_set_stagger(int v) { g_gemm_stagger = v; }
int hq_gemm_get_sched() { return g_gemm_sched; }
void hq_gemm_set_sched(int v) {
  g_gemm_sched = v;
  if (v) {   // allocate the slots now, eagerly: a first GEMM inside a graph capture must not hipMalloc
    std::lock_guard<std::mutex> lock(g_sched_mu);
    (void)sched_pool_locked();
  }
}
