// pg_alignment_list_long_scores: the alignment value of every edge of a CSR list for operands BEYOND 128 positions (up to
// PG_ALN_LONG_MAX_L = 2048), on the strip routines of the long dense kernels (pg_aln_list_long.h is the frame; DESIGN.md
// section 4.29).  All four instances are here: the score modes come from pg_aln_score.h, the global one, AlnGlobalLong, from
// pg_aln_long.hip, included for its mode alone.  The 16-bit cell bounds are the long dense entries' and the caller's to test:
// global W * max(max C, e) + 2 o + 2 e, local min(xl, yl) * max S + 255, semi-global 2 * min(xl, yl) * max S + 255,
// fit o + yl * (e + 2 * max S) + 255, each <= 65 535.  No occupancy is forced: the strip routines need what they need in the
// dense kernels, 2 waves per SIMD (profiles/aln_long_dense.txt, profiles/aln_list_long.txt).
#include "pg_aln_list_long.h"
#include "pg_aln_score.h"
#define ALN_LONG_MODE_ONLY
#include "pg_aln_long.hip"

#define ALN_LIST_LONG_KERNEL(NAME, MODE)                                                                                     \
  __global__ __launch_bounds__(ALN_THREADS) void NAME(                                                                       \
      const u32 *__restrict__ xt, long long n, long long xnpad, int xl, const u32 *__restrict__ yt, long long m, long long ynpad, \
      int yl, const long long *__restrict__ indptr, const int *__restrict__ indices, const void *__restrict__ table, u32 gap,  \
      u32 open, int *__restrict__ scores, u32 *ws) {                                                                         \
    aln_list_long_frame<MODE>(xt, n, xnpad, xl, yt, m, ynpad, yl, indptr, indices, table, gap, open, scores, ws);            \
  }
ALN_LIST_LONG_KERNEL(pg_aln_list_long_global_kernel, AlnGlobalLong)
ALN_LIST_LONG_KERNEL(pg_aln_list_long_local_kernel, AlnLocal)
ALN_LIST_LONG_KERNEL(pg_aln_list_long_semiglobal_kernel, AlnSemiglobal)
ALN_LIST_LONG_KERNEL(pg_aln_list_long_fit_kernel, AlnFit)
#undef ALN_LIST_LONG_KERNEL

extern "C" {

int pg_alignment_list_long_scores(int mode, const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed,
                                  int64_t m, int64_t y_npad, int yl, const int64_t *indptr, const int32_t *indices,
                                  const void *table, int gap, int gap_open, int32_t *scores, void *workspace,
                                  int64_t workspace_bytes, void *stream) {
  const char *who = "pg_alignment_list_long_scores";
  char msg[128];
#define ALN_FAIL(code, what)                          \
  do {                                                \
    snprintf(msg, sizeof(msg), "%s: %s", who, what);  \
    return pg_fail(code, msg);                        \
  } while (0)
  if (mode < 0 || mode > 3) ALN_FAIL(PG_E_BADARG, "mode must be 0 (global), 1 (local), 2 (semi-global) or 3 (fit)");
  if (!x_packed || !y_packed || !indptr || !indices || !table || !scores || n <= 0 || m <= 0 || xl <= 0 || yl <= 0)
    ALN_FAIL(PG_E_BADARG, "bad argument");
  if (xl > ALNG_MAX_L || yl > ALNG_MAX_L) ALN_FAIL(PG_E_TOOLONG, "at most 2048 positions");
  if (gap < 1 || gap > 255) ALN_FAIL(PG_E_BADARG, "gap must be in 1..255");
  if (gap_open < 0 || gap_open > 255) ALN_FAIL(PG_E_BADARG, "gap_open must be in 0..255");
  if (x_npad < n || x_npad % 256 || y_npad < m) ALN_FAIL(PG_E_BADARG, "bad npad");
  if (n > 0x7fffffffll) ALN_FAIL(PG_E_BADARG, "int32 column numbers: at most 2^31 - 1 columns");
  const long long one = aln_long_share(xl);
  if (!workspace || workspace_bytes < one) ALN_FAIL(PG_E_BADARG, "the workspace is smaller than one workgroup's share");
#undef ALN_FAIL
  long long blocks = workspace_bytes / one;                                 // as many workgroups as the workspace holds,
  if (blocks > m) blocks = m;                                               // one per row at the most
  if (blocks > 0x7fffffffll) blocks = 0x7fffffffll;                         // (the loop over the rows covers the rest)
  const AlnListLongCall c = {x_packed, n,      x_npad,   xl,     y_packed,  m,      y_npad, yl, indptr,
                             indices,  table,  gap,      gap_open, scores,  workspace, blocks, stream};
  switch (mode) {
    case 0: return aln_list_long_launch(c, pg_aln_list_long_global_kernel);
    case 1: return aln_list_long_launch(c, pg_aln_list_long_local_kernel);
    case 2: return aln_list_long_launch(c, pg_aln_list_long_semiglobal_kernel);
    default: return aln_list_long_launch(c, pg_aln_list_long_fit_kernel);
  }
}

}  // extern "C"
