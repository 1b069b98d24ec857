// The frame of the PER-PAIR alignment kernels (pg_aln_trace.hip, pg_aln_stats.hip): one pair of a list per
// lane, one wave per workgroup, a grid smaller than the list strides over it.  What those kernels and their entries share
// stands here once: the table in LDS, the lane's pair with the head of an index outside its operand, the clamped lengths,
// and the argument checks of the entries with their messages.
#pragma once
#include "pg_common.h"
#include "pg_aln_trace.h"
#include "../../include/prograph_hip.h"

#define PG_PAIR_WAVE 64

// the 32 x 32 table as int32 in LDS: MINUS the uint8 costs for the global distance, the int8 scores otherwise (pg_aln_trace.h)
__device__ __forceinline__ void pg_pair_table(int *T, int mode, const void *table) {
  for (int k = threadIdx.x; k < 32 * 32; k += PG_PAIR_WAVE)
    T[k] = mode == PG_TR_GLOBAL ? -(int)((const unsigned char *)table)[k] : (int)((const signed char *)table)[k];
  __syncthreads();
}

// the pairs of this lane: p = chunk * 64 + lane over the chunks blockIdx.x, blockIdx.x + gridDim.x, .. of the list; the
// chunk loop is the wave's, `continue` in the body goes on to the next chunk
#define PG_PAIR_FOR(p, npairs, chunks)                                                        \
  for (long long chunk_ = blockIdx.x; chunk_ < (chunks); chunk_ += gridDim.x)                 \
    if (const long long p = chunk_ * PG_PAIR_WAVE + threadIdx.x; p < (npairs))

// Is pair (ix, iy) outside its operands?  Then no operand memory is touched: the head says so (n_ops -1, status 1) and the
// pair's ldo bytes of ops, where the kernel has ops, are zeroed.
__device__ __forceinline__ bool pg_pair_outside(long long ix, long long n, long long iy, long long m, int *hd, unsigned char *op,
                                                long long ldo) {
  if (ix >= 0 && ix < n && iy >= 0 && iy < m) return false;
  hd[0] = hd[1] = hd[2] = hd[3] = hd[4] = hd[6] = 0;
  hd[5] = -1;
  hd[7] = 1;
  if (op)
    for (long long k = 0; k < ldo; ++k) op[k] = 0;
  return true;
}

// the length of a sequence of ng dwords: pg_sub_pack zeroes positions past the width l; the clamp keeps a foreign buffer
// inside the kernel's column and the wave's share
__device__ __forceinline__ int pg_pair_length(const u32 *tok, long long stride, int ng, int l) {
  return min(pg_tr_length(tok, stride, ng), l);
}

static int pg_pair_fail(const char *who, int code, const char *what) {
  char buf[200];
  snprintf(buf, sizeof(buf), "%s: %s", who, what);
  return pg_fail(code, buf);
}

// The argument checks of an entry, after its own mode check: `present` = every pointer it needs is there, max_l the most
// positions.  A trace entry hands in `share`, one wave's bytes of workspace at (xl, yl), with its ldo and workspace_bytes.
static int pg_pair_check(const char *who, bool present, int64_t n, int64_t x_npad, int xl, int64_t m, int64_t y_npad, int yl,
                         int64_t npairs, int gap, int gap_open, int max_l, long long (*share)(int, int) = nullptr, int64_t ldo = 0,
                         int64_t workspace_bytes = 0) {
  if (!present || n <= 0 || m <= 0 || xl <= 0 || yl <= 0 || npairs <= 0) return pg_pair_fail(who, PG_E_BADARG, "bad argument");
  if (xl > max_l || yl > max_l) {
    char what[40];
    snprintf(what, sizeof(what), "at most %d positions", max_l);
    return pg_pair_fail(who, PG_E_TOOLONG, what);
  }
  if (gap < 1 || gap > 255) return pg_pair_fail(who, PG_E_BADARG, "gap must be in 1..255");
  if (gap_open < 0 || gap_open > 255) return pg_pair_fail(who, PG_E_BADARG, "gap_open must be in 0..255");
  if (x_npad < n || y_npad < m) return pg_pair_fail(who, PG_E_BADARG, "bad npad");
  if (share && ldo < (int64_t)xl + yl) return pg_pair_fail(who, PG_E_BADARG, "ldo must be at least xl + yl");
  if (share && workspace_bytes < share(xl, yl)) return pg_pair_fail(who, PG_E_BADARG, "the workspace is smaller than one wave's share");
  return 0;
}
