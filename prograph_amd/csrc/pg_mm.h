// The all-pairs engine, second generation: stage 1 (signature lower bound) on the MATRIX cores.
//
// Replaces the hot loop of Prograph.build_graph (prograph/prograph.py:731-739 and :756-762 of the
// reference): distance(X, batch) -> mask/where or sort -> gather.  Same contract, same per-row
// ownership and output order as pg_nsq.h (one wave owns a pass of rows and sweeps ALL columns in
// ascending order, so eps matches come out in `torch.where` order and kNN lists need no merge);
// what changed is how the ~97 % of pairs that cannot match are rejected.
//
// Stage 1 as an MFMA.  The filter signature of a sequence (its plane-0 bits, 64 positions XOR-folded to
// 54: pg_sig54 in pg_common.h) gives   lb(i,j) = popcount(s_i ^ s_j) <= d(i,j).   That popcount is bilinear:
//     lb = pa_i - sum_k a'_ik * b_jk        a' = +1 / -1 per signature bit of the row,
//                                           b  =  1 /  0 per signature bit of the column,
// so with  A_ik = -a'_ik  (k < 54),  sum_{k >= 54} A_ik = pa_i - bound_i,  B_kj = b_jk,  B_kj = 1 (k >= 54)
//     D = A x B = lb(i,j) - bound_i,        "may be below the row's bound"  <=>  D < 0.
// The instruction is v_mfma_f32_32x32x64_f8f6f4 with FP4 (E2M1) operands: K = 64 elements in the SAME 16
// bytes per lane and the SAME cycles as the int8 32x32x32 form the first version used (31 bits + bias byte;
// tools/ubench/mfma_fp4.hip checks operand layout and exactness: +-1, 0 and the bias values +-{1,2,3,4,6}
// are FP4 numbers, sums of 64 of them are exact in f32, D = 0 comes out as +0).  54 bits instead of 31 cost
// nothing and make unrelated pairs invisible up to bounds of ~12 (one in 3e6 at 10; the 31-bit form let one
// in 2e3 pass at 7): cfg3 3.73 -> 3.55 ms, a 125k x 1M slice 9.3 -> 6.1 ms, and the optimistic kNN cap could
// go from 7 to 10.
// One MFMA evaluates 32 rows x 32 columns.  Up to THREE MFMAs of the hot loop - three column tiles - accumulate into ONE
// set of 16 result registers (the scaled form of the instruction: tile t enters times 2^(8t - 22), the chain starts
// from 2.0, so the three small integers sit in byte fields of the f32 mantissa and "some result is negative" is a test
// of three flag bits: pg_common.h, "chained filter MFMAs"; tools/ubench/mfma_fp4_chain.hip checks exactness and the flag
// identity on the hardware).  The 16 registers of a chain are OR-ed (7 v_bitop3 + 1 v_or) and ONE flag test + scalar
// branch per super-tile decides whether it holds any candidate: ~0.24 VALU instructions per 64 pairs at two row blocks
// (31 per 8192 pairs; one OR tree per MFMA cost 72) instead of ~2.9 (pg_nsq.h), with the multiply-adds on a pipe the
// VALU does not compete for.  At a super-tile with candidates the chains' flagged links are evaluated again, unscaled
// and from zero, for the sign of every result.
// Measured on MI355X for the int8 form (tools/ubench/mfma_s1.hip, N = 200k full sweep): 1.45 ms against
// 3.6 ms for xor + bcnt; insensitive to occupancy (2..8 waves per SIMD) and to how many row blocks share a
// column fragment, i.e. not bound by the 1 KiB-per-MFMA fragment stream from L2.
//   * the row operand A (4 VGPRs) is built once per pass and stays in registers; a row's bias is ten nibbles
//     of it (lane 32+row: top byte of A[2] and A[3]; pg_bias_nibbles).  When a row's distance threshold moves
//     (kNN) the operand is only marked stale and re-encoded for all rows before the next super-tile: a stale
//     bias is looser, never wrong;
//   * the column operand comes from the signature section of the plane buffer (written by pg_pack_planes):
//     per 32 columns one 1 KiB block in MFMA fragment order, so a B operand is a single coalesced
//     global_load_dwordx4; a ring of four tiles is in flight;
//   * candidates (D < 0) are queued as (row, column) in LDS and evaluated exactly 64 at a time, one per lane,
//     with gathered records - as in pg_nsq.h, but now for every candidate (the column records are no longer
//     in registers);
//   * DENSE data (mutant libraries, one big cluster: most pairs pass the plane-0 bound) leaves the MFMA form
//     per run of super-tiles for the folded form (plane folds of all bit planes, B + 1 instructions per 64
//     pairs, hits into the same candidate queue) or, where even that is not selective, the exact form (every
//     distance in place, pg_nsq.h's direct form); see "dense forms" below.
// kNN keeps the optimistic cap / checkpoint / second-phase scheme of pg_nsq.h (exactness argument
// there and in DESIGN.md §4.1); only the representation of the bound changed.
#pragma once
#include "pg_common.h"

typedef int pg_v16i __attribute__((ext_vector_type(16)));

#define PG_MM_RB 32          // rows per pass = M of the MFMA tile
#define PG_MM_QCAP 128       // candidate queue entries per wave: < 64 before a push, <= 64 per push
#define PG_MM_ST 128         // columns per super-tile: 4 MFMA tiles = one direct-form tile (C = 2)
// defaults of the density rules (NsqParams carries them: PG_MM_L1 / PG_MM_RUN override for experiments)
#define PG_MM_DENSE_L1 56    // of 256 lane slots per super-tile with a candidate: leave the MFMA form (tools/dense_knobs.py: 40..64 flat, 96 costs dense data 25 %)
#define PG_MM_DENSE_L2 48    // (unused since the MFMA level 2 was dropped; NsqParams still carries the field)
#define PG_MM_GROUP_ROWS 4    // folded form: rows per group of straight-line code (their folds: 20 SGPRs in flight)
#define PG_MM_DIRECT_RUN 8   // super-tiles of dense form before the MFMA filter is probed again
#define PG_MM_PRIO_STEPS 16  // R = 2: steps of the progress-driven issue priority along a sweep
#define PG_MM_EVICT_MAX 48   // kNN: up to this many rows of a pass that lose their cap at a checkpoint are evicted (NsqParams::mmEvict); more (nearly the
                             // whole pass: data without neighbours inside the cap, e.g. clusters smaller than k + 1): the second phase in the pass
#include "pg_plan.h"        // the entries of delivered keys (sym_entry, sym_group_cap: one text for sweep, merge and host); wants the constants above
#ifndef PG_EXP_SAMETILE
#define PG_EXP_SAMETILE 0   // experiment builds: 1 = every fragment load reads the same super-tile (L1 hits; wrong results)
#endif
#define PG_NSTAT 24          // debug builds (-DPG_MM_STATS): event / cycle counters per launch, then (start, duration) per pass

static_assert(PG_MM_QCAP >= 63 + 64, "a register push adds up to 64 candidates to a queue holding up to 63");
static_assert(PG_QCAP >= 63 + 4 * 2 * PG_PUSH_MAX, "pg_nsq.h kNN queue: a group pushes up to 4 rows x 2 columns x PG_PUSH_MAX");
static_assert(PG_QCAP_EPS >= 63 + 4 * 2 * 64, "pg_nsq.h eps queue: a group pushes up to 4 rows x 2 x 64 lanes");

typedef int pg_v8i __attribute__((ext_vector_type(8)));

// D = A x B over K = 64 FP4 elements (only the first four registers of each operand are read); the result
// comes back as its bit patterns: the filter looks at signs only, and sums of these small integers are exact
__device__ __forceinline__ pg_v16i pg_mfma_fp4(const pg_v4i &a, const pg_v4i &b) {
  const pg_v8i a8 = {a[0], a[1], a[2], a[3], 0, 0, 0, 0}, b8 = {b[0], b[1], b[2], b[3], 0, 0, 0, 0};
  const pg_v16f zero = {0};
  const pg_v16f d = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, zero, 4, 4, 0, 0, 0, 0);
  return __builtin_bit_cast(pg_v16i, d);
}

// a | b | c as v_bitop3_b32 (truth table 0xFE): the 2-cycle issue class of xor / or / bitop3, where v_or3_b32 is in
// the 4-cycle class (profiles/r01_valu_issue_microbench.txt: k_bitop3 2.4-2.9 cycles, k_or3 4.2-4.4)
#ifndef PG_OR3_PLAIN
__device__ __forceinline__ int pg_or3(int a, int b, int c) {
  return (int)__builtin_amdgcn_bitop3_b32((u32)a, (u32)b, (u32)c, 0xFE);
}
#else
__device__ __forceinline__ int pg_or3(int a, int b, int c) { return a | b | c; }
#endif
// median of three unsigned values (sorted insertion: new[i] = med3(old[i-1], key, old[i]))
__device__ __forceinline__ u32 pg_med3(u32 a, u32 b, u32 c) {
  u32 r;
  asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ int pg_or16(const pg_v16i &d) {
  int a = pg_or3(d[0], d[1], d[2]);
  int b = pg_or3(d[3], d[4], d[5]);
  int c = pg_or3(d[6], d[7], d[8]);
  int e = pg_or3(d[9], d[10], d[11]);
  int f = pg_or3(d[12], d[13], d[14]);
  a = pg_or3(a, b, c);
  e = pg_or3(e, f, d[15]);
  return a | e;
}

// Records of up to three chunks (L <= 64 with 5 bit planes): held at 4 waves per SIMD (amdgpu_waves_per_eu(4, 8) =
// 128 VGPRs).  What the compiler reports per instance (-Rpass-analysis=kernel-resource-usage) is committed in
// profiles/r03_kernel_resource_usage.txt: the 64-row kNN instance takes all 128 and spills 5 VGPRs (24 B per lane of
// scratch) in the slow paths; tools/check_ring_asm.py checks on the generated ISA that nothing - no spill, no copy - touches
// a fragment register between its load and the wait in front of the MFMA.
// KL (kNN only): entries of a row's list in LDS.  64 = the list lives across the wave's lanes (lane j = j-th smallest
// key; insertion = one DPP shift, one candidate at a time).  KL < 64 (k + 1 <= KL, PG_MM_KL): the list is KL consecutive
// dwords, RIGHT aligned (the (k+1)-th smallest key, i.e. the row's threshold, is always entry KL-1; unused entries in
// front hold 0), and a flush inserts up to 64 candidates of different rows AT ONCE, one per lane: the winner lane of a row
// reads its list (KL/4 ds_read_b128), new[i] = med3(old[i-1], key, old[i]), writes it back.
// R: row blocks of 32 per pass (1 or 2).  The hot loop is bound by the vector-memory return path (64 B per clock and
// CU: every MFMA needs a fresh 1 KiB fragment; measured ~70 % of that rate, with the loads hitting L1 or L2 alike), so
// R = 2 - two row operands, every fragment feeds two MFMAs - halves that traffic per pair.  Per-row state is lane
// indexed, a wave has 64 lanes: R <= 2.  Short lists only (LDS).
// KS: the symmetric kNN sweep of a self graph (pg_mm_knn_sym_kernel below; the 64-row short-list instance only): a pass is
// (row block, stretch of the super-tiles from the block's own on) out of a plan (SymArgs, pg_common.h), every unordered pair
// is evaluated once - by the pass of its LOWER row, which keeps the pair for its own list (column >= row) and delivers
// it to the log of the higher row's group (SymArgs::lowKeys: one entry per pair, d < cap only).  Bounds stay at the optimistic cap for the
// whole sweep (no publish, no checkpoints, no second phase: the owner of a pair cannot know the other row's threshold;
// what the cap hides the merge detects, as for column pieces), lists go to SymArgs::partial, pg_knn_sym_merge_kernel
// (pg_api.hip) makes the rows' results.
template <class M, int MODE, int KL = 64, int R = 1>
// (records of four chunks - byte alphabets at L <= 64 - in the 32-row short-list kNN instance: held at three waves per SIMD,
//  168 VGPRs; left alone it takes 173 since the eviction code: two waves, N = 200k 2.05 -> 2.5 ms)
__global__ __launch_bounds__(PG_WG_THREADS) __attribute__((amdgpu_waves_per_eu(
    M::Q <= 3 ? 4 : ((M::Q == 4 && MODE == PG_MODE_KNN && KL < 64 && R == 1) ? 3 : 1), 8))) void pg_mm_kernel(const NsqParams p) {
  constexpr bool KS = false;
#include "pg_mm_body.h"
}
// the symmetric kNN sweep (KS above): a kernel of its own name - records of up to three chunks, lists of PG_MM_KL entries
template <class M>
__global__ __launch_bounds__(PG_WG_THREADS) __attribute__((amdgpu_waves_per_eu(4, 8))) void pg_mm_knn_sym_kernel(const NsqParams p) {
  static_assert(M::Q <= 3, "records of up to three chunks");
  constexpr int MODE = PG_MODE_KNN, KL = PG_MM_KL, R = 2;
  constexpr bool KS = true;
#include "pg_mm_body.h"
}
#undef PG_ST
