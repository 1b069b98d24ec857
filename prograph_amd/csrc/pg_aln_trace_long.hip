// ALIGNMENT TRACEBACK BEYOND 128 POSITIONS: pg_aln_trace.hip's canonical alignment for operands of up to
// 2048 positions.  The same shape - one pair per lane, one wave per workgroup, the lane's row of H and E in LDS as int32
// col[j - j0 - 1][lane], F, the diagonal and the running end cell in registers, the int32 table (negated for the distance)
// in LDS - but the row in LDS is one STRIP of 128 columns: a lane runs strip s over all rows i = 1..len x, then strip
// s + 1.  128 * 64 * 8 + 32 * 64 * 4 + 4096 = 77 824 bytes, two workgroups per compute unit.  Between strips the lane keeps
// one boundary column, H[i][j0] and F[i][j0], in the wave's share of the workspace as bnd[i - 1][H | F][lane] (a wave's
// access is one 256-byte line), read at row i for the strip's left edge and overwritten at row i with its right edge; the
// direction dwords go to ws[((i - 1) * ND + w) * 64 + lane] as in pg_aln_trace.hip, ND = ceil(yl / 8) <= 256.  A lane reads
// back only what it stored itself, in program order: no fence.  Lanes loop to their own len x and their own number of
// strips (wave loops to the longest under the EXEC mask); the end cell follows pg_tr_end_take, whose rule does not depend
// on the order of the sweep.  Cells are int32, so no table or penalty is excluded (pg_aln_trace.h).
#include "pg_common.h"
#include "pg_aln_trace.h"
#include "../../include/prograph_hip.h"

#define TR_WAVE 64

static long long trace_long_share(int xl, int yl) {                        // bytes: direction bits + boundary column
  return (long long)TR_WAVE * xl * ((yl + 7) / 8) * 4 + (long long)TR_WAVE * xl * 8;
}

__global__ __launch_bounds__(TR_WAVE) void pg_aln_trace_long_kernel(
    int mode, const u32 *__restrict__ xt, long long n, long long xnpad, int xl, const u32 *__restrict__ yt, long long m,
    long long ynpad, int yl, const int *__restrict__ xi, const int *__restrict__ yi, long long npairs, const void *__restrict__ table,
    int e, int oe, int *__restrict__ head, unsigned char *__restrict__ ops, long long ldo, u32 *__restrict__ ws, long long chunks) {
  __shared__ int colH[PG_TR_STRIP * TR_WAVE];
  __shared__ int colE[PG_TR_STRIP * TR_WAVE];
  __shared__ u32 ytok[(PG_TR_STRIP / 4) * TR_WAVE];
  __shared__ int T[32 * 32];
  const int lane = threadIdx.x;
  for (int k = lane; k < 32 * 32; k += TR_WAVE)
    T[k] = mode == PG_TR_GLOBAL ? -(int)((const unsigned char *)table)[k] : (int)((const signed char *)table)[k];
  __syncthreads();
  const int xg = (xl + 3) >> 2, yg = (yl + 3) >> 2, nd = (yl + 7) >> 3;     // <= 512, 512, 256 (the host checks)
  u32 *dir = ws + (long long)blockIdx.x * xl * (nd + 2) * TR_WAVE + lane;   // this wave's share, this lane's dwords
  int *bnd = (int *)(dir + (long long)xl * nd * TR_WAVE);                   // after the direction bits: [i - 1][H | F][lane]

  for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    const long long p = chunk * TR_WAVE + lane;
    if (p >= npairs) continue;
    int *hd = head + p * 8;
    unsigned char *op = ops + p * ldo;
    const long long ix = xi[p], iy = yi[p];
    if (ix < 0 || ix >= n || iy < 0 || iy >= m) {                           // no operand memory is touched
      hd[0] = hd[1] = hd[2] = hd[3] = hd[4] = hd[6] = 0;
      hd[5] = -1;
      hd[7] = 1;
      for (long long k = 0; k < ldo; ++k) op[k] = 0;
      continue;
    }
    const u32 *xb = xt + ix, *yb = yt + iy;
    // pg_sub_pack zeroes positions past the width; the clamps keep a foreign buffer inside col[] and the wave's share
    const int lx = min(pg_tr_length(xb, xnpad, xg), xl), ly = min(pg_tr_length(yb, ynpad, yg), yl);
    pg_tr_end end;
    pg_tr_end0(mode, lx, ly, &end);
    if (mode == PG_TR_FIT) pg_tr_end0_fit(ly, e, oe, &end);
    int last = 0;                                                           // H[len x][len y] once the last strip is through
    for (int j0 = 0; j0 < ly; j0 += PG_TR_STRIP) {
      const int sg = min(PG_TR_STRIP / 4, yg - (j0 >> 2));
      for (int g = 0; g < sg; ++g) ytok[g * TR_WAVE + lane] = yb[(long long)((j0 >> 2) + g) * ynpad];
      pg_tr_strip_row0(mode, j0, ly, e, oe, colH + lane, colE + lane, TR_WAVE);
      const bool more = ly > j0 + PG_TR_STRIP;                              // the right edge is another strip's left edge
      int diag = pg_tr_border(mode, j0, e, oe);                             // H[0][j0]
      u32 xw = 0;
      for (int i = 1; i <= lx; ++i) {
        if (((i - 1) & 3) == 0) xw = xb[(long long)((i - 1) >> 2) * xnpad];
        int *b = bnd + (long long)(i - 1) * 2 * TR_WAVE;
        const int left = j0 ? b[0] : pg_tr_border_x(mode, i, e, oe), fin = j0 ? b[TR_WAVE] : PG_TR_NEG;
        int rh, rf;
        pg_tr_row_strip(mode, i, lx, ly, j0, e, oe, T + 32 * (int)((xw >> (8 * ((i - 1) & 3))) & 31u), ytok + lane, TR_WAVE,
                        colH + lane, colE + lane, TR_WAVE, dir + (long long)(i - 1) * nd * TR_WAVE, TR_WAVE, &end, left, fin, diag,
                        &rh, &rf);
        diag = left;
        last = rh;
        if (more) {
          b[0] = rh;
          b[TR_WAVE] = rf;
        }
      }
    }
    hd[0] = mode != PG_TR_GLOBAL ? end.best : -(lx == 0 ? pg_tr_border(mode, ly, e, oe) : ly == 0 ? pg_tr_border(mode, lx, e, oe) : last);
    hd[7] = 0;
    pg_tr_walk_room(mode, lx, ly, end.i, end.j, xb, xnpad, yb, ynpad, dir, nd, TR_WAVE, op, ldo, 2 * PG_TR_LONG_MAX_L, hd);
  }
}

static int trace_fail(const char *who, int code, const char *what) {
  char buf[200];
  snprintf(buf, sizeof(buf), "%s: %s", who, what);
  return pg_fail(code, buf);
}

// the checks and the launch of both entries; `mode` is already checked
static int trace_run(const char *who, int mode, const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed,
    int64_t m, int64_t y_npad, int yl, const int32_t *xi, const int32_t *yi, int64_t npairs, const void *table, int gap, int gap_open,
    int32_t *head, uint8_t *ops, int64_t ldo, void *workspace, int64_t workspace_bytes, void *stream) {
  if (!x_packed || !y_packed || !xi || !yi || !table || !head || !ops || !workspace || n <= 0 || m <= 0 || xl <= 0 || yl <= 0 ||
      npairs <= 0)
    return trace_fail(who, PG_E_BADARG, "bad argument");
  if (xl > PG_TR_LONG_MAX_L || yl > PG_TR_LONG_MAX_L) return trace_fail(who, PG_E_TOOLONG, "at most 2048 positions");
  if (gap < 1 || gap > 255) return trace_fail(who, PG_E_BADARG, "gap must be in 1..255");
  if (gap_open < 0 || gap_open > 255) return trace_fail(who, PG_E_BADARG, "gap_open must be in 0..255");
  if (x_npad < n || y_npad < m) return trace_fail(who, PG_E_BADARG, "bad npad");
  if (ldo < (int64_t)xl + yl) return trace_fail(who, PG_E_BADARG, "ldo must be at least xl + yl");
  const long long one = trace_long_share(xl, yl);
  if (workspace_bytes < one) return trace_fail(who, PG_E_BADARG, "the workspace is smaller than one wave's share");
  const long long chunks = (npairs + TR_WAVE - 1) / TR_WAVE;
  long long blocks = workspace_bytes / one;                                 // as many waves as the workspace holds
  if (blocks > chunks) blocks = chunks;
  if (blocks > 0x7fffffffll) blocks = 0x7fffffffll;
  pg_aln_trace_long_kernel<<<dim3((unsigned)blocks), dim3(TR_WAVE), 0, (hipStream_t)stream>>>(
      mode, (const u32 *)x_packed, n, x_npad, xl, (const u32 *)y_packed, m, y_npad, yl, xi, yi, npairs, table, gap,
      gap_open + gap, head, ops, ldo, (u32 *)workspace, chunks);
  return pg_launched(who);
}

extern "C" {

int pg_alignment_trace_long_workspace(int xl, int yl, int64_t *bytes_per_wave) {
  if (xl <= 0 || yl <= 0 || !bytes_per_wave) return pg_fail(PG_E_BADARG, "pg_alignment_trace_long_workspace: bad argument");
  if (xl > PG_TR_LONG_MAX_L || yl > PG_TR_LONG_MAX_L)
    return pg_fail(PG_E_TOOLONG, "pg_alignment_trace_long_workspace: at most 2048 positions");
  *bytes_per_wave = trace_long_share(xl, yl);
  return 0;
}

int pg_alignment_trace_long(int mode, const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
    int64_t y_npad, int yl, const int32_t *xi, const int32_t *yi, int64_t npairs, const void *table, int gap, int gap_open,
    int32_t *head, uint8_t *ops, int64_t ldo, void *workspace, int64_t workspace_bytes, void *stream) {
  if (mode != PG_ALN_TRACE_GLOBAL && mode != PG_ALN_TRACE_LOCAL && mode != PG_ALN_TRACE_SEMIGLOBAL)
    return trace_fail("pg_alignment_trace_long", PG_E_BADARG, "mode must be 0 (global), 1 (local) or 2 (semi-global)");
  return trace_run("pg_alignment_trace_long", mode, x_packed, n, x_npad, xl, y_packed, m, y_npad, yl, xi, yi, npairs, table, gap,
                   gap_open, head, ops, ldo, workspace, workspace_bytes, stream);
}

// mode PG_TR_FIT: all of y within any substring of x (pg_aln_trace.h).  The entry above goes on rejecting mode 3.
int pg_alignment_fit_trace_long(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
    int64_t y_npad, int yl, const int32_t *xi, const int32_t *yi, int64_t npairs, const void *table, int gap, int gap_open,
    int32_t *head, uint8_t *ops, int64_t ldo, void *workspace, int64_t workspace_bytes, void *stream) {
  return trace_run("pg_alignment_fit_trace_long", PG_TR_FIT, x_packed, n, x_npad, xl, y_packed, m, y_npad, yl, xi, yi, npairs, table, gap,
                   gap_open, head, ops, ldo, workspace, workspace_bytes, stream);
}

}  // extern "C"
