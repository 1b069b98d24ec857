// ALIGNMENT STATISTICS: the head of pg_alignment_trace - score, ranges, n_ops, identities - of a list of
// (x row, y row) pairs WITHOUT the alignment's columns: what a percent-identity cut needs of every edge of a graph.  The
// forward recurrence carries the counts of the canonical path (pg_aln_stats.h), so there are no direction bits, no walk, no
// ops and no workspace: 32 bytes out per pair.
//
// §4.20's shape: one pair per lane, one wave per workgroup.  The lane's row lives in LDS as 16-byte cells col[j][lane] =
// (H, E, wH, wE) - one 128-bit LDS read and one write per cell, a lane's own len y is a plain address - F, the diagonal and
// their words in registers, the lane's y tokens and the table (int32, negated for the distance) in LDS too.  The column is
// as long as the y operand is WIDE, so the kernel is compiled for widths of up to 32, 64 and 128 positions:
// (YMAX + 1) * 64 * 16 + YMAX / 4 * 64 * 4 + 4096 = 39 936, 74 752 and 144 384 bytes, four, two and ONE workgroup per
// compute unit.  Lanes loop to their own lengths, which the compiler turns into wave loops to the longest under the EXEC
// mask.  A grid smaller than the list strides over it.
#include "pg_common.h"
#include "pg_aln_stats.h"
#include "../../include/prograph_hip.h"

#define ST_WAVE 64
#define ST_MAX_BLOCKS 1024              // one workgroup per compute unit is resident: four rounds of the device, the rest stride

template <int YMAX>
__global__ __launch_bounds__(ST_WAVE) void pg_aln_stats_kernel(
    int mode, const u32 *__restrict__ xt, long long n, long long xnpad, int xl, const u32 *__restrict__ yt, long long m,
    long long ynpad, int yl, const int *__restrict__ xi, const int *__restrict__ yi, long long npairs, const void *__restrict__ table,
    int e, int oe, int *__restrict__ head, long long chunks) {
  __shared__ pg_st_cell col[(YMAX + 1) * ST_WAVE];
  __shared__ u32 ytok[(YMAX / 4) * ST_WAVE];
  __shared__ int T[32 * 32];
  const int lane = threadIdx.x;
  for (int k = lane; k < 32 * 32; k += ST_WAVE)
    T[k] = mode == PG_TR_GLOBAL ? -(int)((const unsigned char *)table)[k] : (int)((const signed char *)table)[k];
  __syncthreads();
  const int xg = (xl + 3) >> 2, yg = (yl + 3) >> 2;                         // <= 32, YMAX / 4 (the host checks xl, chooses YMAX >= yl)

  for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    const long long p = chunk * ST_WAVE + lane;
    if (p >= npairs) continue;
    int *hd = head + p * 8;
    const long long ix = xi[p], iy = yi[p];
    if (ix < 0 || ix >= n || iy < 0 || iy >= m) {                           // no operand memory is touched
      hd[0] = hd[1] = hd[2] = hd[3] = hd[4] = hd[6] = 0;
      hd[5] = -1;
      hd[7] = 1;
      continue;
    }
    const u32 *xb = xt + ix, *yb = yt + iy;
    for (int g = 0; g < yg; ++g) ytok[g * ST_WAVE + lane] = yb[(long long)g * ynpad];
    // pg_sub_pack zeroes positions past the width; the clamps keep a foreign buffer inside col[]
    const int lx = min(pg_tr_length(xb, xnpad, xg), xl), ly = min(pg_tr_length(ytok + lane, ST_WAVE, yg), yl);
    pg_tr_end end;
    u32 endw;
    pg_st_row0(mode, lx, ly, e, oe, col + lane, ST_WAVE, &end, &endw);
    u32 xw = 0;
    for (int i = 1; i <= lx; ++i) {
      if (((i - 1) & 3) == 0) xw = xb[(long long)((i - 1) >> 2) * xnpad];   // one dword of x per four rows
      const int x = (int)((xw >> (8 * ((i - 1) & 3))) & 31u);
      pg_st_row(mode, i, lx, ly, e, oe, T + 32 * x, x, ytok + lane, ST_WAVE, col + lane, ST_WAVE, &end, &endw);
    }
    const pg_st_cell last = col[ly * ST_WAVE + lane];
    pg_st_head(mode == PG_TR_GLOBAL ? -last.h : end.best, &end, mode == PG_TR_GLOBAL ? last.wh : endw, hd);
    hd[7] = 0;
  }
}

extern "C" {

int pg_alignment_stats(int mode, const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
    int64_t y_npad, int yl, const int32_t *xi, const int32_t *yi, int64_t npairs, const void *table, int gap, int gap_open,
    int32_t *head, void *stream) {
  const char *who = "pg_alignment_stats";
  char buf[200];
  const char *what = nullptr;
  int code = PG_E_BADARG;
  if (mode != PG_TR_GLOBAL && mode != PG_TR_LOCAL && mode != PG_TR_SEMIGLOBAL && mode != PG_TR_FIT)
    what = "mode must be 0 (global), 1 (local), 2 (semi-global) or 3 (fit)";
  else if (!x_packed || !y_packed || !xi || !yi || !table || !head || n <= 0 || m <= 0 || xl <= 0 || yl <= 0 || npairs <= 0)
    what = "bad argument";
  else if (xl > PG_TR_MAX_L || yl > PG_TR_MAX_L) {
    what = "at most 128 positions";
    code = PG_E_TOOLONG;
  } else if (gap < 1 || gap > 255)
    what = "gap must be in 1..255";
  else if (gap_open < 0 || gap_open > 255)
    what = "gap_open must be in 0..255";
  else if (x_npad < n || y_npad < m)
    what = "bad npad";
  if (what) {
    snprintf(buf, sizeof(buf), "%s: %s", who, what);
    return pg_fail(code, buf);
  }
  const long long chunks = (npairs + ST_WAVE - 1) / ST_WAVE;
  const long long blocks = chunks < ST_MAX_BLOCKS ? chunks : ST_MAX_BLOCKS;
#define ST_LAUNCH(YMAX)                                                                                                   \
  pg_aln_stats_kernel<YMAX><<<dim3((unsigned)blocks), dim3(ST_WAVE), 0, (hipStream_t)stream>>>(                            \
      mode, (const u32 *)x_packed, n, x_npad, xl, (const u32 *)y_packed, m, y_npad, yl, xi, yi, npairs, table, gap,        \
      gap_open + gap, head, chunks)
  if (yl <= 32) ST_LAUNCH(32);
  else if (yl <= 64) ST_LAUNCH(64);
  else ST_LAUNCH(PG_TR_MAX_L);
#undef ST_LAUNCH
  return pg_launched(who);
}

}  // extern "C"
