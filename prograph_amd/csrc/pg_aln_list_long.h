// The LONG LIST frame of the gapped-alignment score kernels (pg_alignment_list_long_scores): the strip
// routines of the long dense kernels, mode.strip<NC, LAST>(q, x, wsb, j0, rest, best) of pg_aln_long.hip and pg_aln_score.h,
// on the edges of a CSR list instead of the column tiles of a block.  Up to ALNG_MAX_L positions.  It is the strip-mined row
// loop of aln_long_frame (pg_aln_frame.h) with the column tile replaced by a row's edge list, as aln_list_frame
// (pg_aln_list.h) did for aln_short_frame.
//
// Shape.  Workgroup b takes the rows b, b + gridDim.x, ... of Y, one at a time.  A row whose list is empty costs nothing but
// the two words of indptr.  Otherwise the workgroup stages the row's tokens and finds its length as aln_long_frame does,
// and cuts its profile into strips of ALN_STRIP positions, up to ALN_ROWS consecutive strips (one GROUP) in the 8 LDS slots.
// The row's list is cut into 64-entry chunks and walked in ROUNDS of four chunks, one per wave: in round k wave w takes
// chunk 4 k + w, lane t of it entry e = indptr[row] + 64 (4 k + w) + t.  AlnX.lane is the entry's COLUMN and xb the
// operand's base, so aln_x_word reads the lane's own sequence whichever column that is; lx comes from the packed dwords,
// lxmax from a shuffle, ly stays wave-uniform.  A lane past the end of the list, or whose entry lies outside 0..n-1 (the -1
// of an unfilled kNN slot), has lx = 0 and column 0: it runs no cell, touches no workspace line and stores INT32_MIN, or
// nothing past the end.
//
// The boundary column.  The layout is aln_long_frame's: [i][thread] per workgroup in flight, aln_long_share(xl) bytes each,
// slice b for workgroup b.  The strip routines address a step's line as bd[x.lane], and x.lane is the column here, so the
// lane is handed ITS OWN base, wsb + (thread - column): bd[x.lane] is then wsb[i][thread] exactly, inside the slice whatever
// the column is.  A lane reads back only what the same thread stored, and only at steps i < lx of the same chunk.
// Two conditions hold the frame together:
//   1. The workspace holds ONE boundary column per lane, so a wave finishes every strip of a chunk - every group - before
//      it starts its next chunk: the loop over the groups is inside the loop over the rounds.
//   2. Every __syncthreads() is reached the same number of times by all four waves.  A row of more than 1024 positions has
//      a second group of strips, so its profiles are rebuilt inside every round (barrier, build, barrier, strips) - and a
//      wave with no chunk in that round (chunks not a multiple of 4) still takes those barriers: everything that decides
//      whether a barrier is reached (the row's list length, its strip count) is uniform over the workgroup, and only the
//      strips and the store are under `active`.  A row of up to 1024 positions has one group: one build per row, before
//      the rounds, and the waves run free until the next row.
//
// 16-bit cells: the bounds are the long dense kernels' (pg_aln_long.hip, pg_aln_semiglobal.hip, pg_aln_fit.hip); the kernel
// tests none of them, the caller does.
#pragma once
#include <climits>
#include "pg_aln_frame.h"
#include "pg_aln_list_long_walk.h"      // the walk's arithmetic, aln_ll_*: plain functions that tests/capi_list_long enumerates

#define ALN_LIST_WAVES (ALN_THREADS / 64)
static_assert(ALN_LL_WAVES == ALN_LIST_WAVES && ALN_LL_STRIP == ALN_STRIP && ALN_LL_SLOTS == ALN_ROWS, "pg_aln_list_long_walk.h");

struct AlnListLongCall {           // the arguments of pg_alignment_list_long_scores, checked
  const void *x;
  int64_t n, x_npad;
  int xl;
  const void *y;
  int64_t m, y_npad;
  int yl;
  const int64_t *indptr;
  const int32_t *indices;
  const void *table;
  int gap, gap_open;
  int32_t *scores;
  void *ws;
  int64_t blocks;                  // workgroups: min(rows, shares in the workspace)
  void *stream;
};

// the profiles of strips s0 .. s0 + nb - 1 of the staged row into the slots 0 .. nb - 1 (aln_long_frame's build)
template <bool SCORE>
__device__ __forceinline__ void aln_ll_build(unsigned char *Q, const unsigned char *cs, const u32 *yrow, int ly, int s0, int nb, int tid) {
  for (int i = tid; i < nb * 32 * 32; i += ALN_THREADS) {
    const int g = i & 31, a = (i >> 5) & 31, slot = i >> 10;
    const int gy = (s0 + slot) * (ALN_STRIP / 4) + g;                       // < 512
    *(u32 *)(Q + slot * ALN_QBYTES + a * ALN_QSTRIDE + 4 * g) = aln_profile<SCORE>(cs + a * ALN_CSTRIDE, yrow[gy], ly - 4 * gy);
  }
}

template <class M>
__device__ __forceinline__ void aln_list_long_frame(const u32 *__restrict__ xt, long long n, long long xnpad, int xl,
                                                    const u32 *__restrict__ yt, long long m, long long ynpad, int yl,
                                                    const long long *__restrict__ indptr, const int *__restrict__ indices,
                                                    const void *__restrict__ table, u32 gap, u32 open, int *__restrict__ scores,
                                                    u32 *ws) {
  __shared__ __attribute__((aligned(16))) unsigned char Q[ALN_ROWS * ALN_QBYTES];
  __shared__ u32 yrow[ALNG_MAX_L / 4];
  __shared__ unsigned char cs[32 * ALN_CSTRIDE];
  __shared__ int ylen;
  __shared__ int smin, smax;
  const int tid = threadIdx.x;
  const int xg = (xl + 3) >> 2, yg = (yl + 3) >> 2;                         // <= 512 dwords each (the host checks)
  u32 bias = 0, top = 0;
  if (M::SCORE) bias = aln_score_table<M::TOP>((const signed char *)table, cs, &smin, &smax, tid, &top);
  else aln_cost_table((const unsigned char *)table, cs, tid);               // (the row's barriers come before its first reader)
  const M mode(AlnParams{gap, open, xl, yl, 0, bias, top});

  // Everything that steers the walk is a scalar, as in aln_list_frame; addresses formed from the lane are formed chunk by chunk.
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  u32 *wsb = ws + (long long)blockIdx.x * (xg * 4 * ALN_THREADS);          // this workgroup's boundary column
  for (long long row = blockIdx.x; row < m; row += gridDim.x) {
    const long long e0 = indptr[row], e1 = indptr[row + 1];                 // uniform over the workgroup
    const int chunks = aln_ll_chunks(e1 - e0);                              // (a list of 2^37 entries fits no device)
    if (chunks == 0) continue;                                              // no list: no tokens, no profile, no barrier - for every wave
    __syncthreads();                                                        // the previous row's readers of Q / yrow / ylen are done
    if (tid == 0) ylen = 0;
    __syncthreads();
    for (int g = tid; g < ALNG_MAX_L / 4; g += ALN_THREADS) {
      const u32 w = g < yg ? yt[(long long)g * ynpad + row] : 0u;
      yrow[g] = w;
      if (w) atomicMax(&ylen, aln_len(w, g));
    }
    __syncthreads();
    const int ly = __builtin_amdgcn_readfirstlane(ylen);
    const int ns = aln_ll_strips(ly);
    const bool regroup = aln_ll_groups(ns) > 1;                             // more than one group: the build is inside the rounds
    if (!regroup) {
      aln_ll_build<M::SCORE>(Q, cs, yrow, ly, 0, ns, tid);
      __syncthreads();                                                      // the row's last barrier: Q is read-only from here
    }
    const int rounds = aln_ll_rounds(chunks);
    for (int round = 0; round < rounds; ++round) {
      const int left = aln_ll_left(e1 - e0, round, wave);                   // this wave's chunk: its entries, 1..64, or 0 for none
      const bool active = left > 0;                                         // wave-uniform; decides no barrier
      const long long eb = e0 + ((long long)(round * ALN_LIST_WAVES + wave) << 6);      // the chunk's first entry
      int l = lane;
      asm volatile("" : "+v"(l));
      const int col = l < left ? (indices + eb)[l] : -1;
      const bool valid = col >= 0 && col < n;
      const int c = valid ? col : 0;                                        // a column of the operand whatever the entry says
      int lx = 0;
      if (active)
        for (int g = 0; g < xg; ++g) lx = max(lx, aln_len(valid ? (xt + (long long)g * xnpad)[c] : 0u, g));
      int lxmax = lx;
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) lxmax = max(lxmax, __builtin_amdgcn_ds_bpermute((l ^ s) << 2, lxmax));
      const AlnX x{xt, xnpad, c, lx, __builtin_amdgcn_readfirstlane(lxmax)};
      u32 *wl = wsb + (tid - c);                                            // wl[i * ALN_THREADS + x.lane] is wsb[i][tid]
      u32 best = mode.first(ly, lx);                                        // carried from strip to strip
      for (int s0 = 0; s0 < ns; s0 += ALN_ROWS) {
        const int nb = min(ALN_ROWS, ns - s0);
        if (regroup) {
          __syncthreads();                                                  // the previous group's profiles are read, by every wave
          aln_ll_build<M::SCORE>(Q, cs, yrow, ly, s0, nb, tid);
          __syncthreads();
        }
        if (active) {
          for (int s = s0; s < s0 + nb; ++s) {
            const unsigned char *q = Q + (s - s0) * ALN_QBYTES;
            const int j0 = s * ALN_STRIP;
            if (s < ns - 1) {
              best = mode.template strip<8, false>(q, x, wl, j0, 0, best);
              continue;
            }
            const int rest = ly - j0;                                       // 1..128
#define ALN_LAST(NC) best = mode.template strip<NC, true>(q, x, wl, j0, rest, best)
            ALN_NC_SWITCH((rest + 15) >> 4, (void)0, ALN_LAST)
#undef ALN_LAST
          }
        }
      }
      l = lane;
      asm volatile("" : "+v"(l));
      if (l < left) (scores + eb)[l] = valid ? mode.template value<int>(best) : INT_MIN;
    }
  }
}

using AlnListLongKernel = void(const u32 *, long long, long long, int, const u32 *, long long, long long, int, const long long *,
                               const int *, const void *, u32, u32, int *, u32 *);

// a persistent grid: one workgroup per share of the workspace, at most one per row
static inline int aln_list_long_launch(const AlnListLongCall &c, AlnListLongKernel *k) {
  const dim3 grid((unsigned)c.blocks), block(ALN_THREADS);
  k<<<grid, block, 0, (hipStream_t)c.stream>>>((const u32 *)c.x, c.n, c.x_npad, c.xl, (const u32 *)c.y, c.m, c.y_npad, c.yl,
                                               (const long long *)c.indptr, c.indices, c.table, (u32)c.gap, (u32)c.gap_open,
                                               c.scores, (u32 *)c.ws);
  return pg_launched("pg_alignment_list_long_scores");
}
