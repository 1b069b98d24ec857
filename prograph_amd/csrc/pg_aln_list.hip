// pg_alignment_list_scores: the alignment value of every edge of a CSR list, on the row routines of the dense kernels
// (pg_aln_list.h is the frame).  All four instances are here: the score modes come from
// pg_aln_score.h, the global one, AlnAffine, from pg_aln_affine.hip, included for its mode alone.  The 16-bit cell bounds at these widths (<= 128 positions) are the short dense
// kernels' own: global 128 * 255 + 4 * 255 < 35 000 (pg_aln_affine.hip), local 128 * 127 + 255 (pg_aln_local.hip),
// semi-global 2 * 128 * 127 + 255 = 32 767 (pg_aln_semiglobal.hip); fit alone needs its caller's predicate
// gap_open + yl * (gap + 2 * max S) + 255 <= 65 535 (pg_aln_fit.hip).
#include "pg_aln_list.h"
#include "pg_aln_score.h"
#define ALN_AFFINE_MODE_ONLY
#include "pg_aln_affine.hip"

#define ALN_LIST_KERNEL(NAME, MODE)                                                                                          \
  __global__ __launch_bounds__(ALN_THREADS) __attribute__((amdgpu_waves_per_eu(3))) void NAME(                                \
      const u32 *__restrict__ xt, long long n, long long xnpad, int xl, const u32 *__restrict__ yt, long long m, long long ynpad, \
      int yl, const long long *__restrict__ indptr, const int *__restrict__ indices, const void *__restrict__ score, u32 gap,  \
      u32 open, int *__restrict__ scores) {                                                                                  \
    aln_list_frame<MODE>(xt, n, xnpad, xl, yt, m, ynpad, yl, indptr, indices, score, gap, open, scores);                      \
  }
ALN_LIST_KERNEL(pg_aln_list_affine_kernel, AlnAffine)
ALN_LIST_KERNEL(pg_aln_list_local_kernel, AlnLocal)
ALN_LIST_KERNEL(pg_aln_list_semiglobal_kernel, AlnSemiglobal)
ALN_LIST_KERNEL(pg_aln_list_fit_kernel, AlnFit)
#undef ALN_LIST_KERNEL

extern "C" {

int pg_alignment_list_scores(int mode, const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                             int64_t y_npad, int yl, const int64_t *indptr, const int32_t *indices, const void *table, int gap,
                             int gap_open, int32_t *scores, void *stream) {
  const char *who = "pg_alignment_list_scores";
  char msg[128];
#define ALN_FAIL(code, what)                          \
  do {                                                \
    snprintf(msg, sizeof(msg), "%s: %s", who, what);  \
    return pg_fail(code, msg);                        \
  } while (0)
  if (mode < 0 || mode > 3) ALN_FAIL(PG_E_BADARG, "mode must be 0 (global), 1 (local), 2 (semi-global) or 3 (fit)");
  if (!x_packed || !y_packed || !indptr || !indices || !table || !scores || n <= 0 || m <= 0 || xl <= 0 || yl <= 0)
    ALN_FAIL(PG_E_BADARG, "bad argument");
  if (xl > ALN_MAX_L || yl > ALN_MAX_L) ALN_FAIL(PG_E_TOOLONG, "at most 128 positions");
  if (gap < 1 || gap > 255) ALN_FAIL(PG_E_BADARG, "gap must be in 1..255");
  if (gap_open < 0 || gap_open > 255) ALN_FAIL(PG_E_BADARG, "gap_open must be in 0..255");
  if (x_npad < n || x_npad % 256 || y_npad < m) ALN_FAIL(PG_E_BADARG, "bad npad");
  if (n > 0x7fffffffll) ALN_FAIL(PG_E_BADARG, "int32 column numbers: at most 2^31 - 1 columns");
  if ((m + ALN_ROWS - 1) / ALN_ROWS > 0x7fffffffll) ALN_FAIL(PG_E_BADARG, "too many rows for one launch");
#undef ALN_FAIL
  const AlnListCall c = {x_packed, n, x_npad, xl, y_packed, m, y_npad, yl, indptr, indices, table, gap, gap_open, scores, stream};
  switch (mode) {
    case 0: return aln_list_launch(c, pg_aln_list_affine_kernel);
    case 1: return aln_list_launch(c, pg_aln_list_local_kernel);
    case 2: return aln_list_launch(c, pg_aln_list_semiglobal_kernel);
    default: return aln_list_launch(c, pg_aln_list_fit_kernel);
  }
}

}  // extern "C"
