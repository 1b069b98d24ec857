// The LIST frame of the gapped-alignment score kernels (pg_alignment_list_scores): the row routines of
// the dense kernels, mode.row<NC>(q, x, ly) of pg_aln_affine.hip and pg_aln_score.h, on the edges of a CSR list instead of
// the column tiles of a block.  Up to ALN_MAX_L positions.
//
// Shape.  Workgroup b owns the ALN_ROWS rows of Y from b * ALN_ROWS: it builds their byte query profiles into the 8 LDS
// slots exactly as aln_short_frame does, and after the one barrier that ends the build its four waves go their own ways.
// The work of the 8 rows is cut into items (row, 64-entry chunk of that row's list); wave w takes the items w, w + 4, ... of
// that order.  In an item lane t takes entry e = indptr[row] + 64 * chunk + t: AlnX.lane is the entry's COLUMN and xb the
// operand's base, so aln_x_word - a wave-uniform base plus the lane - reads the lane's own sequence whichever column that
// is.  The gather costs the cell loop nothing: it was one dword load per four outer steps before and it is one now; only
// its addresses no longer share cache lines.  The lane finds its length from the packed dwords, the wave's longest comes
// from aln_x's shuffle, ly stays wave-uniform (one row per item) for the chunk switch and the last-column masks, and
// one int32 per lane is stored, coalesced in edge order.  A lane past the end of the list, or whose entry lies outside
// 0..n-1 (the -1 of an unfilled kNN slot), has lx = 0 and column 0: it loads column 0's dwords with the wave, runs no cell
// and stores INT32_MIN, or nothing past the end.
//
// Limit.  A wave serves ONE row at a time, so a chunk uses min(entries left, 64) of its 64 lanes: a 16-edge list runs at a
// quarter of the lanes.  Rows are not packed into one wave: ly would no longer be wave-uniform.
#pragma once
#include <climits>
#include "pg_aln_frame.h"

#define ALN_LIST_WAVES (ALN_THREADS / 64)

struct AlnListCall {               // the arguments of pg_alignment_list_scores, checked
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
  void *stream;
};

template <class M>
__device__ __forceinline__ void aln_list_frame(const u32 *__restrict__ xt, long long n, long long xnpad, int xl,
                                               const u32 *__restrict__ yt, long long m, long long ynpad, int yl,
                                               const long long *__restrict__ indptr, const int *__restrict__ indices,
                                               const void *__restrict__ table, u32 gap, u32 open, int *__restrict__ scores) {
  __shared__ __attribute__((aligned(16))) unsigned char Q[ALN_ROWS * ALN_QBYTES];
  __shared__ u32 ytile[ALN_ROWS][ALN_MAX_L / 4];
  __shared__ unsigned char cs[32 * ALN_CSTRIDE];
  __shared__ int ylen[ALN_ROWS];
  __shared__ int smin, smax;
  const int tid = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * ALN_ROWS;
  const int xg = (xl + 3) >> 2, yg = (yl + 3) >> 2;                         // <= 32 dwords each (the host checks)

  // the profiles of the 8 rows: aln_short_frame's build
  for (int i = tid; i < ALN_ROWS * (ALN_MAX_L / 4); i += ALN_THREADS) {
    const int r = i >> 5, g = i & 31;
    ytile[r][g] = (row0 + r < m && g < yg) ? yt[(long long)g * ynpad + row0 + r] : 0u;
  }
  u32 bias = 0, top = 0;
  if (M::SCORE) {
    bias = aln_score_table<M::TOP>((const signed char *)table, cs, &smin, &smax, tid, &top);      // its barriers cover ytile
  } else {
    aln_cost_table((const unsigned char *)table, cs, tid);
    __syncthreads();
  }
  if (tid < ALN_ROWS) {
    int len = 0;
    for (int g = 0; g < ALN_MAX_L / 4; ++g) len = max(len, aln_len(ytile[tid][g], g));
    ylen[tid] = len;
  }
  if (M::SCORE) __syncthreads();                                            // the masked gather reads ylen
  for (int i = tid; i < ALN_ROWS * 32 * 32; i += ALN_THREADS) {
    const int g = i & 31, a = (i >> 5) & 31, r = i >> 10;
    *(u32 *)(Q + r * ALN_QBYTES + a * ALN_QSTRIDE + 4 * g) =
        aln_profile<M::SCORE>(cs + a * ALN_CSTRIDE, ytile[r][g], M::SCORE ? ylen[r] - 4 * g : 4);
  }
  __syncthreads();                                                          // the last barrier: Q and ylen are read-only from here

  // Everything that steers the walk is a scalar: 64-bit values that the compiler would compare in vector registers, and
  // addresses formed from the lane and hoisted out of the loops (the shuffle's, the list's, the result's), would stay alive
  // across the row routine, which has no register to spare (profiles/aln_list.txt).
  const int lane = tid & 63;
  const int rows = (int)min((long long)ALN_ROWS, m - row0);                 // >= 1: the grid covers rows of Y only
  int next = __builtin_amdgcn_readfirstlane(tid >> 6);                      // this wave's next item, counted from the row's chunk 0
  M mode(AlnParams{gap, open, xl, yl, 0, bias, top});
  for (int r = 0; r < rows; ++r) {
    const long long e0 = indptr[row0 + r], e1 = indptr[row0 + r + 1];       // wave-uniform
    const int chunks = (int)((e1 - e0 + 63) >> 6);                          // (a list of 2^37 entries fits no device)
    if (next >= chunks) {                                                   // none of this row's items is this wave's (an empty list too)
      next -= chunks;
      continue;
    }
    const int ly = __builtin_amdgcn_readfirstlane(ylen[r]);
    const unsigned char *q = Q + r * ALN_QBYTES;
    int chunk = next;
    for (; chunk < chunks; chunk += ALN_LIST_WAVES) {
      const long long eb = e0 + ((long long)chunk << 6);                    // the chunk's first entry
      const int left = (int)min(64ll, e1 - eb);                             // its entries, 1..64
      int l = lane;
      asm volatile("" : "+v"(l));                                           // addresses from the lane are formed here, chunk by chunk
      const int col = l < left ? (indices + eb)[l] : -1;
      const bool valid = col >= 0 && col < n;
      const int c = valid ? col : 0;                                        // a column of the operand whatever the entry says
      int lx = 0;
      for (int g = 0; g < xg; ++g) lx = max(lx, aln_len(valid ? (xt + (long long)g * xnpad)[c] : 0u, g));
      int lxmax = lx;
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) lxmax = max(lxmax, __builtin_amdgcn_ds_bpermute((l ^ s) << 2, lxmax));
      const AlnX x{xt, xnpad, c, lx, __builtin_amdgcn_readfirstlane(lxmax)};
      mode.begin_row(ly);
      u32 d;
#define ALN_ROW(NC) d = mode.template row<NC>(q, x, ly)
      ALN_NC_SWITCH((ly + 15) >> 4, d = mode.first(0, x.lx), ALN_ROW)
#undef ALN_ROW
      l = lane;
      asm volatile("" : "+v"(l));                                           // and here again: nothing of them lives across the row
      if (l < left) (scores + eb)[l] = valid ? mode.template value<int>(d) : INT_MIN;
    }
    next = chunk - chunks;
  }
}

using AlnListKernel = void(const u32 *, long long, long long, int, const u32 *, long long, long long, int, const long long *,
                           const int *, const void *, u32, u32, int *);

// one workgroup per 8 rows of Y (the entry has checked that they fit a grid)
static inline int aln_list_launch(const AlnListCall &c, AlnListKernel *k) {
  const dim3 grid((unsigned)((c.m + ALN_ROWS - 1) / ALN_ROWS)), block(ALN_THREADS);
  k<<<grid, block, 0, (hipStream_t)c.stream>>>((const u32 *)c.x, c.n, c.x_npad, c.xl, (const u32 *)c.y, c.m, c.y_npad, c.yl,
                                               (const long long *)c.indptr, c.indices, c.table, (u32)c.gap, (u32)c.gap_open,
                                               c.scores);
  return pg_launched("pg_alignment_list_scores");
}
