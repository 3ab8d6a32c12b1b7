// The tile core of the 256-row MFMA GEMMs, once.  Device code only, private to csrc/kernels: the bf16 NT kernels
// (gemm_nt_v1 / _vs / _v2 / _v3.hip) take all of it, gemm_fp8.hip and gemm_tn.hip the parts that fit their kernels
// (typedefs, barrier, descriptor word, mfma16, the half stager).  Everything here is __forceinline__ and compiles
// to the code the kernels had with the text written out in each — which depends on the FORM of a function (by
// value or by reference, function or lambda), not only on its text: tools/isa_diff.py is the check when this
// changes, and profiles/gemm_split/README.md lists the forms that failed it and what therefore stayed per kernel.
//
// STAGE / WAIT TABLE of the pipelined kernels (v2, v3, gemm_fp8.hip's two, gemm_tn.hip's: same halves, same waits).
// A K-tile is four 16 KiB halves (A0 A1 B0 B1: 128 rows × 128 B each) in one of two LDS buffers.  Wave (wm, wn)
// owns four 64×32 quadrants (mh, nh): rows mh·128 + wm·64 + [0,64), cols wn·64 + nh·32 + [0,32), so quadrant
// (mh, nh) reads exactly A-half mh and B-half nh.  One K-tile = 2 phases of 32 MFMAs per wave, each a (fragment
// reads + stage | barrier | MFMAs | barrier) pair; the two wave rows (wm) run one barrier apart, so one row's
// MFMAs cover the other's reads:
//   P01: reads B(nh 0), A(mh 0), B(nh 1); stages A1 of K-tile t+1   | MFMAs (0,0) (0,1)
//   P23: reads A(mh 1); stages A0, B0, B1 of K-tile t+2              | MFMAs (1,1) (1,0)
// Every half is staged by all 8 waves (16 rows each) and read 4-6 barrier intervals later; each wave's counted
// wait retires its own rows at least one barrier before ANY wave reads them.  A half is re-staged only after
// both rows have read it (A1 of buffer b1 two intervals after its last read, the others one).
// Waits (vmcnt retires in issue order, so a wait names how many YOUNGER ops may stay in flight):
//   P01 waits for A1 of K-tile t (staged in P01 of t-1).  Younger: P23(t-1)'s 3 halves = 6 ops (at t = 0 the
//     prologue's K-tile-1 halves) -> vmcnt(6); nothing younger on the last K-tile -> vmcnt(0).  K-tile t's
//     A0 B0 B1 were retired by P23(t-1)'s wait.
//   P23 waits for K-tile t+1's A0 B0 B1, read by both wave rows in their next P01.  Younger: this P01's A1 = 2
//     ops -> vmcnt(2), else vmcnt(0).  BOTH rows wait: each half's rows are staged by all 8 waves, so a wave of
//     row 0 reads rows of the other row-0 waves, whose P01 wait is in the same barrier interval as that read (an
//     earlier schedule let row 0 skip this wait and relied on the DMA landing within the 6 intervals since issue).
// The persistent kernels run the table across the tile seam: past a tile's end the stages come from the next
// tile's K-tile 0 (t+1 == nt, t+2 == nt), and at t = 0 of a following tile the previous epilogue's E vm ops per
// lane (issued after the K-tile-1 halves) are younger too: vmcnt(6 + E), vmcnt(2 + E).
#pragma once
#include "hq_common.h"

namespace hq_tile {

constexpr int BM = 256;
constexpr int BK = 64;
constexpr int kThreads = 512;

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) void g_void;
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

// word 3 of a raw buffer descriptor (gfx9: DATA_FORMAT = 32, no swizzle, no index stride): offsets are plain
// bytes and a load past num_records returns zeros
constexpr int kRawBufferWord3 = 0x00020000;

__device__ __forceinline__ f32x4_t mfma16(const bf16x8_t& a, const bf16x8_t& b, const f32x4_t& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// Raw workgroup barrier: no __syncthreads (its fence would drain the LDS-DMA in flight); the empty asm
// statements keep hipcc from moving memory operations across it.
__device__ __forceinline__ void bar() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// The 16-B slot swizzle of the bf16 kernels' 128-B LDS rows, slot' = slot ^ ((row >> 1) & 7), is written out in the
// three functions that apply it: stage_panel and lane_src_offset on the source, frag on the read.

// Issue the LDS-DMA of one [ROWS × 64] bf16 panel (rows of 128 B) into lds (+ byte offset).
// Each wave-instruction moves 8 rows (64 lanes × 16 B); this wave handles `n_instr` of them
// starting at panel row `row0`.
template <int N_INSTR>
__device__ __forceinline__ void stage_panel(const uint16_t* __restrict__ g, int ld, int row0, int k0, char* lds_base,
                                            int lane) {
  const int r_in = lane >> 3;          // 0..7 row within the 8-row piece
  const int slot = lane & 7;           // 16-B slot in the 128-B LDS row (lane-linear destination)
#pragma unroll
  for (int i = 0; i < N_INSTR; ++i) {
    const int row = row0 + i * 8 + r_in;
    const int src_slot = slot ^ ((row >> 1) & 7);
    const uint16_t* src = g + (size_t)row * ld + k0 + src_slot * 8;
    char* dst = lds_base + (size_t)(row0 + i * 8) * 128;  // wave-uniform; lane L lands at dst + 16 L
    __builtin_amdgcn_global_load_lds((g_void*)src, (lds_void*)dst, 16, 0, 0);
  }
}

// 16-B fragment read of LDS row `row`, k-slot `slot` (8 bf16 = 16 B), undoing the source swizzle.
__device__ __forceinline__ bf16x8_t frag(const char* panel, int row, int slot) {
  const int off = row * 128 + ((slot ^ ((row >> 1) & 7)) << 4);
  return *reinterpret_cast<const bf16x8_t*>(panel + off);
}

// Buffer-load staging: a lane's byte offset into a bf16 panel (rows of ld elements) for the 8-row piece that starts
// at panel row row0: row row0 + lane / 8, the 16-B source slot that the swizzle places at this lane's LDS slot.  The
// offsets of a wave's pieces are the same for every half and K-tile (the swizzle depends on row bits 1..3 only), so
// those advance in the scalar offset.  The operands come by reference and the loop over the pieces stays with
// the kernel: of the forms tried, the only one that leaves the kernels' code as it was (profiles/gemm_split).
__device__ __forceinline__ int lane_src_offset(const int& row0, const int& lane, const int& ld) {
  const int row = row0 + (lane >> 3);
  const int src_slot = (lane & 7) ^ ((row >> 1) & 7);
  return (row * ld + src_slot * 8) * 2;
}

// One 16 KiB half (128 rows × 128 B) of K-tile `kt` of a 256-row panel into its LDS image at `panel`: wave w
// stages rows w·16 … +15 of it with two buffer-load-to-LDS instructions; the half and K-tile advance is the
// scalar offset.  rs spans the block's row panel (rows of ld elements of ES bytes), vo = the lane's two piece
// offsets.  For the persistent kernels (v3, gemm_fp8p_kernel); in the per-tile ones (v2, gemm_fp8_kernel) it
// changes the scalar schedule around the loads, so they keep a lambda of their own.  ld and wave_u by reference,
// as those kernels' lambdas captured them.
template <int ES>
__device__ __forceinline__ void stage_half(__amdgpu_buffer_rsrc_t rs, const int (&vo)[2], const int& ld, int half, int kt,
                                           char* panel, const int& wave_u) {
  char* dst = panel + (half * 128 + wave_u * 16) * 128;
  const int so = half * 128 * ld * ES + kt * 128;
#pragma unroll
  for (int i = 0; i < 2; ++i) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(dst + i * 8 * 128), 16, vo[i], so, 0, 0);
}

// The A fragments of m-half mh (both k-steps of a K-tile) out of the A panel image pa, and the 16-MFMA product of
// quadrant (mh, nh); fr = lane & 15, fq = lane >> 4.  Operands SWAPPED (B fragment as the MFMA's A input): the
// accumulator holds Cᵀ, a lane owns 4 consecutive n of one m.  acc is [mh·4 + i][nh·2 + j].  The lane
// coordinates come by reference, as the kernels' lambdas captured them: by value the kernels' code changes.
__device__ __forceinline__ void readA(bf16x8_t (&af)[2][4], const char* pa, int mh, const int& wm, const int& fr,
                                      const int& fq) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int i = 0; i < 4; ++i) af[ks][i] = frag(pa, mh * 128 + wm * 64 + i * 16 + fr, ks * 4 + fq);
}
// (readB, the B fragments of n-half nh at rows wn·64 + nh·32 + j·16 + fr, stays a lambda in v2 and v3: as a
// function, in every parameter form tried, one v_bitop3 of each kernel comes out with its operands swapped.)
__device__ __forceinline__ void mma(f32x4_t (&acc)[8][4], const bf16x8_t (&af)[2][4], const bf16x8_t (&bf)[2][2], int mh,
                                    int nh) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[mh * 4 + i][nh * 2 + j] = mfma16(bf[ks][j], af[ks][i], acc[mh * 4 + i][nh * 2 + j]);
  __builtin_amdgcn_s_setprio(0);
}

}  // namespace hq_tile
