// ALIGNMENT STATISTICS: the head of pg_alignment_trace - score, ranges, n_ops, identities - of a list of
// (x row, y row) pairs WITHOUT the alignment's columns: what a percent-identity cut needs of every edge of a graph.  The
// forward recurrence carries the counts of the canonical path (pg_aln_stats.h), so there are no direction bits, no walk, no
// ops and no workspace: 32 bytes out per pair.
//
// §4.20's shape on its frame (pg_aln_pair.h): one pair per lane, one wave per workgroup.  The lane's row lives in LDS as
// 16-byte cells col[j][lane] = (H, E, wH, wE) - one 128-bit LDS read and one write per cell, a lane's own len y is a plain
// address - F, the diagonal and their words in registers, the lane's y tokens and the table (int32, negated for the
// distance) in LDS too.  The column is as long as the y operand is WIDE, so the kernel is compiled for widths of up to 32,
// 64 and 128 positions: (YMAX + 1) * 64 * 16 + YMAX / 4 * 64 * 4 + 4096 = 39 936, 74 752 and 144 384 bytes, four, two and
// ONE workgroup per compute unit.  Lanes loop to their own lengths, which the compiler turns into wave loops to the longest
// under the EXEC mask.  A grid smaller than the list strides over it.
#include "pg_aln_pair.h"
#include "pg_aln_stats.h"

#define ST_WAVE PG_PAIR_WAVE
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
  pg_pair_table(T, mode, table);
  const int xg = (xl + 3) >> 2, yg = (yl + 3) >> 2;                         // <= 32, YMAX / 4 (the host checks xl, chooses YMAX >= yl)

  PG_PAIR_FOR(p, npairs, chunks) {
    int *hd = head + p * 8;
    const long long ix = xi[p], iy = yi[p];
    if (pg_pair_outside(ix, n, iy, m, hd, nullptr, 0)) continue;
    const u32 *xb = xt + ix, *yb = yt + iy;
    for (int g = 0; g < yg; ++g) ytok[g * ST_WAVE + lane] = yb[(long long)g * ynpad];
    const int lx = pg_pair_length(xb, xnpad, xg, xl), ly = pg_pair_length(ytok + lane, ST_WAVE, yg, yl);
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
  if (mode != PG_TR_GLOBAL && mode != PG_TR_LOCAL && mode != PG_TR_SEMIGLOBAL && mode != PG_TR_FIT)
    return pg_pair_fail(who, PG_E_BADARG, "mode must be 0 (global), 1 (local), 2 (semi-global) or 3 (fit)");
  const int rc = pg_pair_check(who, x_packed && y_packed && xi && yi && table && head, n, x_npad, xl, m, y_npad, yl, npairs, gap,
                               gap_open, PG_TR_MAX_L);
  if (rc) return rc;
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
