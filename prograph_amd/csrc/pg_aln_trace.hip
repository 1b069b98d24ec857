// ALIGNMENT TRACEBACK: the canonical alignment of a list of (x row, y row) pairs under
// `alignment`, `local_alignment`, `semiglobal_alignment` or `fit_alignment` - which symbols pair, which stay unaligned,
// where the alignment sits.  A traceback is wanted per graph edge, after the all-pairs sweep has chosen the edges, so this
// kernel is exact and general (any two lengths in one wave, int32 cells: no table or penalty is excluded) rather than at
// the VALU floor of the scoring kernels.
//
// One pair per lane, one wave per workgroup (pg_aln_pair.h).  The lane's row of H and E lives in LDS as int32
// col[j - j0 - 1][lane], one STRIP of 128 columns (a lane's own len y is a plain address, consecutive lanes hit consecutive
// banks), F, the diagonal and the running end cell in registers, the y tokens and the int32 table in LDS too:
// 128 * 64 * 8 + 32 * 64 * 4 + 4096 = 77 824 bytes, two workgroups per compute unit.  The rows and the walk are
// pg_aln_trace.h's routines; lanes loop to their own lengths and their own number of strips, which the compiler turns into
// wave loops to the longest under the EXEC mask.  Each cell leaves a direction nibble, eight to a dword, stored
// lane-interleaved - ws[((i - 1) * ND + w) * 64 + lane], ND = ceil(yl / 8), one 256-byte line per wave store - in the
// wave's share of the caller's workspace; the same lane then walks back over its own dwords (program order: no fence) and
// writes its row of `ops` and `head`.
//
// LONG = false, up to 128 positions: the one strip j0 = 0.  All of the lane's y tokens stay in LDS for the length and the
// walk, and the share is the direction bits alone, 64 * xl * ND * 4 bytes.
// LONG = true, up to 2048: a lane runs strip s over all rows i = 1..len x, then strip s + 1.  Between strips it keeps one
// boundary column, H[i][j0] and F[i][j0], behind the direction bits of the share as bnd[i - 1][H | F][lane] (64 * xl * 8
// bytes more; a wave's access is one 256-byte line), read at row i for the strip's left edge and overwritten at row i with
// its right edge.  The end cell follows pg_tr_end_take, whose rule does not depend on the order of the sweep.
#include "pg_aln_pair.h"

#define TR_WAVE PG_PAIR_WAVE

template <bool LONG>
static long long trace_share(int xl, int yl) {                              // bytes: direction bits (+ boundary column)
  return (long long)TR_WAVE * xl * ((yl + 7) / 8) * 4 + (LONG ? (long long)TR_WAVE * xl * 8 : 0);
}

template <bool LONG>
__global__ __launch_bounds__(TR_WAVE) void pg_aln_trace_kernel(
    int mode, const u32 *__restrict__ xt, long long n, long long xnpad, int xl, const u32 *__restrict__ yt, long long m,
    long long ynpad, int yl, const int *__restrict__ xi, const int *__restrict__ yi, long long npairs, const void *__restrict__ table,
    int e, int oe, int *__restrict__ head, unsigned char *__restrict__ ops, long long ldo, u32 *__restrict__ ws, long long chunks) {
  __shared__ int colH[PG_TR_STRIP * TR_WAVE];
  __shared__ int colE[PG_TR_STRIP * TR_WAVE];
  __shared__ u32 ytok[(PG_TR_STRIP / 4) * TR_WAVE];
  __shared__ int T[32 * 32];
  const int lane = threadIdx.x;
  pg_pair_table(T, mode, table);
  const int xg = (xl + 3) >> 2, yg = (yl + 3) >> 2, nd = (yl + 7) >> 3;     // the host checks xl, yl <= 128 or 2048
  u32 *dir = ws + (long long)blockIdx.x * xl * (nd + (LONG ? 2 : 0)) * TR_WAVE + lane;   // this wave's share, this lane's dwords
  int *bnd = (int *)(dir + (long long)xl * nd * TR_WAVE);                   // LONG: [i - 1][H | F][lane]

  PG_PAIR_FOR(p, npairs, chunks) {
    int *hd = head + p * 8;
    unsigned char *op = ops + p * ldo;
    const long long ix = xi[p], iy = yi[p];
    if (pg_pair_outside(ix, n, iy, m, hd, op, ldo)) continue;
    const u32 *xb = xt + ix, *yb = yt + iy;
    if (!LONG)
      for (int g = 0; g < yg; ++g) ytok[g * TR_WAVE + lane] = yb[(long long)g * ynpad];
    const u32 *yw = LONG ? yb : ytok + lane;                                // all of y, for the length and the walk
    const long long yws = LONG ? ynpad : TR_WAVE;
    const int lx = pg_pair_length(xb, xnpad, xg, xl), ly = pg_pair_length(yw, yws, yg, yl);
    pg_tr_end end;
    pg_tr_end0(mode, lx, ly, &end);
    if (mode == PG_TR_FIT) pg_tr_end0_fit(ly, e, oe, &end);
    int last = 0;                                                           // H[len x][len y] once the last strip is through
    for (int j0 = 0; j0 < ly; j0 += PG_TR_STRIP) {
      if (LONG) {
        const int sg = min(PG_TR_STRIP / 4, yg - (j0 >> 2));
        for (int g = 0; g < sg; ++g) ytok[g * TR_WAVE + lane] = yb[(long long)((j0 >> 2) + g) * ynpad];
      }
      pg_tr_row0(mode, j0, ly, e, oe, colH + lane, colE + lane, TR_WAVE);
      const bool first = !LONG || j0 == 0;                                  // the left edge is the border
      const bool more = LONG && ly > j0 + PG_TR_STRIP;                      // the right edge is another strip's left edge
      int diag = pg_tr_border(mode, j0, e, oe);                             // H[0][j0]
      u32 xw = 0;
      for (int i = 1; i <= lx; ++i) {
        if (((i - 1) & 3) == 0) xw = xb[(long long)((i - 1) >> 2) * xnpad];   // one dword of x per four rows
        int *b = bnd + (long long)(i - 1) * 2 * TR_WAVE;
        const int left = first ? pg_tr_border_x(mode, i, e, oe) : b[0], fin = first ? PG_TR_NEG : b[TR_WAVE];
        int rh, rf;
        pg_tr_row(mode, i, lx, ly, j0, e, oe, T + 32 * (int)((xw >> (8 * ((i - 1) & 3))) & 31u), ytok + lane, TR_WAVE, colH + lane,
                  colE + lane, TR_WAVE, dir + (long long)(i - 1) * nd * TR_WAVE, TR_WAVE, &end, left, fin, diag, &rh, &rf);
        diag = left;
        last = rh;
        if (more) {
          b[0] = rh;
          b[TR_WAVE] = rf;
        }
      }
      if (!LONG) break;                                                     // ly <= PG_TR_STRIP: j0 = 0 folds away
    }
    hd[0] = mode == PG_TR_GLOBAL ? pg_tr_global(lx, ly, e, oe, last) : end.best;
    hd[7] = 0;
    pg_tr_walk_room(mode, lx, ly, end.i, end.j, xb, xnpad, yw, yws, dir, nd, TR_WAVE, op, ldo,
                    2 * (LONG ? PG_TR_LONG_MAX_L : PG_TR_MAX_L), hd);
  }
}

// the checks and the launch of every entry; `mode` is already checked
template <bool LONG>
static int trace_run(const char *who, int mode, const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed,
    int64_t m, int64_t y_npad, int yl, const int32_t *xi, const int32_t *yi, int64_t npairs, const void *table, int gap, int gap_open,
    int32_t *head, uint8_t *ops, int64_t ldo, void *workspace, int64_t workspace_bytes, void *stream) {
  const int rc = pg_pair_check(who, x_packed && y_packed && xi && yi && table && head && ops && workspace, n, x_npad, xl, m, y_npad, yl,
                               npairs, gap, gap_open, LONG ? PG_TR_LONG_MAX_L : PG_TR_MAX_L, trace_share<LONG>, ldo, workspace_bytes);
  if (rc) return rc;
  const long long chunks = (npairs + TR_WAVE - 1) / TR_WAVE;
  long long blocks = workspace_bytes / trace_share<LONG>(xl, yl);           // as many waves as the workspace holds
  if (blocks > chunks) blocks = chunks;
  if (blocks > 0x7fffffffll) blocks = 0x7fffffffll;
  pg_aln_trace_kernel<LONG><<<dim3((unsigned)blocks), dim3(TR_WAVE), 0, (hipStream_t)stream>>>(
      mode, (const u32 *)x_packed, n, x_npad, xl, (const u32 *)y_packed, m, y_npad, yl, xi, yi, npairs, table, gap,
      gap_open + gap, head, ops, ldo, (u32 *)workspace, chunks);
  return pg_launched(who);
}

template <bool LONG>
static int trace_workspace(const char *who, int xl, int yl, int64_t *bytes_per_wave) {
  if (xl <= 0 || yl <= 0 || !bytes_per_wave) return pg_pair_fail(who, PG_E_BADARG, "bad argument");
  if (xl > (LONG ? PG_TR_LONG_MAX_L : PG_TR_MAX_L) || yl > (LONG ? PG_TR_LONG_MAX_L : PG_TR_MAX_L))
    return pg_pair_fail(who, PG_E_TOOLONG, LONG ? "at most 2048 positions" : "at most 128 positions");
  *bytes_per_wave = trace_share<LONG>(xl, yl);
  return 0;
}

static bool trace_mode_ok(int mode) { return mode == PG_ALN_TRACE_GLOBAL || mode == PG_ALN_TRACE_LOCAL || mode == PG_ALN_TRACE_SEMIGLOBAL; }

#define TRACE_ARGS                                                                                                          \
  const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m, int64_t y_npad, int yl,         \
      const int32_t *xi, const int32_t *yi, int64_t npairs, const void *table, int gap, int gap_open, int32_t *head,        \
      uint8_t *ops, int64_t ldo, void *workspace, int64_t workspace_bytes, void *stream
#define TRACE_PASS \
  x_packed, n, x_npad, xl, y_packed, m, y_npad, yl, xi, yi, npairs, table, gap, gap_open, head, ops, ldo, workspace, workspace_bytes, stream
#define TRACE_BAD_MODE "mode must be 0 (global), 1 (local) or 2 (semi-global)"

extern "C" {

int pg_alignment_trace_workspace(int xl, int yl, int64_t *bytes_per_wave) {
  return trace_workspace<false>("pg_alignment_trace_workspace", xl, yl, bytes_per_wave);
}

int pg_alignment_trace_long_workspace(int xl, int yl, int64_t *bytes_per_wave) {
  return trace_workspace<true>("pg_alignment_trace_long_workspace", xl, yl, bytes_per_wave);
}

int pg_alignment_trace(int mode, TRACE_ARGS) {
  if (!trace_mode_ok(mode)) return pg_pair_fail("pg_alignment_trace", PG_E_BADARG, TRACE_BAD_MODE);
  return trace_run<false>("pg_alignment_trace", mode, TRACE_PASS);
}

int pg_alignment_trace_long(int mode, TRACE_ARGS) {
  if (!trace_mode_ok(mode)) return pg_pair_fail("pg_alignment_trace_long", PG_E_BADARG, TRACE_BAD_MODE);
  return trace_run<true>("pg_alignment_trace_long", mode, TRACE_PASS);
}

// mode PG_TR_FIT: all of y within any substring of x (pg_aln_trace.h).  The entries above go on rejecting mode 3.
int pg_alignment_fit_trace(TRACE_ARGS) { return trace_run<false>("pg_alignment_fit_trace", PG_TR_FIT, TRACE_PASS); }

int pg_alignment_fit_trace_long(TRACE_ARGS) { return trace_run<true>("pg_alignment_fit_trace_long", PG_TR_FIT, TRACE_PASS); }

}  // extern "C"
