// ALIGNMENT TRACEBACK: the canonical alignment of a list of (x row, y row) pairs under `alignment`,
// `local_alignment` or `semiglobal_alignment` - which symbols pair, which stay unaligned, where the alignment sits.  A
// traceback is wanted per graph edge, after the all-pairs sweep has chosen the edges, so this kernel is exact and general
// (any two lengths up to 128 in one wave) rather than at the VALU floor of the scoring kernels.
//
// One pair per lane, one wave per workgroup.  The lane's row of H and E lives in LDS as int32 col[j][lane] (a lane's own
// len y is a plain address, consecutive lanes hit consecutive banks), F and the diagonal in registers, the lane's y tokens
// and the table (as int32, negated for the distance: pg_aln_trace.h) in LDS too: 129 * 64 * 8 + 32 * 64 * 4 + 4096 =
// 78 336 bytes, two workgroups per compute unit.  The rows and the walk are pg_aln_trace.h's routines; lanes loop to their
// own lengths, which the compiler turns into wave loops to the longest under the EXEC mask.  Each cell leaves a direction
// nibble, eight to a dword, stored lane-interleaved - ws[(i * ND + w) * 64 + lane], one 256-byte line per wave store -
// in the wave's share of the caller's workspace, 64 * xl * ceil(yl / 8) * 4 bytes; the same lane then walks back over its
// own dwords (program order: no fence) and writes its row of `ops` and `head`.  A grid smaller than the list strides over it.
#include "pg_common.h"
#include "pg_aln_trace.h"
#include "../../include/prograph_hip.h"

#define TR_WAVE 64

__global__ __launch_bounds__(TR_WAVE) void pg_aln_trace_kernel(
    int mode, const u32 *__restrict__ xt, long long n, long long xnpad, int xl, const u32 *__restrict__ yt, long long m,
    long long ynpad, int yl, const int *__restrict__ xi, const int *__restrict__ yi, long long npairs, const void *__restrict__ table,
    int e, int oe, int *__restrict__ head, unsigned char *__restrict__ ops, long long ldo, u32 *__restrict__ ws, long long chunks) {
  __shared__ int colH[(PG_TR_MAX_L + 1) * TR_WAVE];
  __shared__ int colE[(PG_TR_MAX_L + 1) * TR_WAVE];
  __shared__ u32 ytok[(PG_TR_MAX_L / 4) * TR_WAVE];
  __shared__ int T[32 * 32];
  const int lane = threadIdx.x;
  for (int k = lane; k < 32 * 32; k += TR_WAVE)
    T[k] = mode == PG_TR_GLOBAL ? -(int)((const unsigned char *)table)[k] : (int)((const signed char *)table)[k];
  __syncthreads();
  const int xg = (xl + 3) >> 2, yg = (yl + 3) >> 2, nd = (yl + 7) >> 3;     // <= 32, 32, 16 (the host checks)
  u32 *dir = ws + (long long)blockIdx.x * xl * nd * TR_WAVE + lane;         // this wave's share, this lane's dwords

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
    for (int g = 0; g < yg; ++g) ytok[g * TR_WAVE + lane] = yb[(long long)g * ynpad];
    // pg_sub_pack zeroes positions past the width; the clamps keep a foreign buffer inside col[] and the wave's share
    const int lx = min(pg_tr_length(xb, xnpad, xg), xl), ly = min(pg_tr_length(ytok + lane, TR_WAVE, yg), yl);
    pg_tr_end end;
    pg_tr_row0(mode, lx, ly, e, oe, colH + lane, colE + lane, TR_WAVE, &end);
    for (int i = 1; i <= lx; ++i)
      pg_tr_row(mode, i, lx, ly, e, oe, T + 32 * pg_tr_token(xb, xnpad, i - 1), ytok + lane, TR_WAVE, colH + lane, colE + lane,
                TR_WAVE, dir + (long long)(i - 1) * nd * TR_WAVE, TR_WAVE, &end);
    hd[0] = mode == PG_TR_GLOBAL ? -colH[ly * TR_WAVE + lane] : end.best;
    hd[7] = 0;
    pg_tr_walk(mode, lx, ly, end.i, end.j, xb, xnpad, ytok + lane, TR_WAVE, dir, nd, TR_WAVE, op, ldo, hd);
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
  if (xl > PG_TR_MAX_L || yl > PG_TR_MAX_L) return trace_fail(who, PG_E_TOOLONG, "at most 128 positions");
  if (gap < 1 || gap > 255) return trace_fail(who, PG_E_BADARG, "gap must be in 1..255");
  if (gap_open < 0 || gap_open > 255) return trace_fail(who, PG_E_BADARG, "gap_open must be in 0..255");
  if (x_npad < n || y_npad < m) return trace_fail(who, PG_E_BADARG, "bad npad");
  if (ldo < (int64_t)xl + yl) return trace_fail(who, PG_E_BADARG, "ldo must be at least xl + yl");
  const long long one = (long long)TR_WAVE * xl * ((yl + 7) / 8) * 4;
  if (workspace_bytes < one) return trace_fail(who, PG_E_BADARG, "the workspace is smaller than one wave's share");
  const long long chunks = (npairs + TR_WAVE - 1) / TR_WAVE;
  long long blocks = workspace_bytes / one;                                 // as many waves as the workspace holds
  if (blocks > chunks) blocks = chunks;
  if (blocks > 0x7fffffffll) blocks = 0x7fffffffll;
  pg_aln_trace_kernel<<<dim3((unsigned)blocks), dim3(TR_WAVE), 0, (hipStream_t)stream>>>(
      mode, (const u32 *)x_packed, n, x_npad, xl, (const u32 *)y_packed, m, y_npad, yl, xi, yi, npairs, table, gap,
      gap_open + gap, head, ops, ldo, (u32 *)workspace, chunks);
  return pg_launched(who);
}

extern "C" {

int pg_alignment_trace_workspace(int xl, int yl, int64_t *bytes_per_wave) {
  if (xl <= 0 || yl <= 0 || !bytes_per_wave) return pg_fail(PG_E_BADARG, "pg_alignment_trace_workspace: bad argument");
  if (xl > PG_TR_MAX_L || yl > PG_TR_MAX_L) return pg_fail(PG_E_TOOLONG, "pg_alignment_trace_workspace: at most 128 positions");
  *bytes_per_wave = (int64_t)TR_WAVE * xl * ((yl + 7) / 8) * 4;
  return 0;
}

int pg_alignment_trace(int mode, const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
    int64_t y_npad, int yl, const int32_t *xi, const int32_t *yi, int64_t npairs, const void *table, int gap, int gap_open,
    int32_t *head, uint8_t *ops, int64_t ldo, void *workspace, int64_t workspace_bytes, void *stream) {
  if (mode != PG_ALN_TRACE_GLOBAL && mode != PG_ALN_TRACE_LOCAL && mode != PG_ALN_TRACE_SEMIGLOBAL)
    return trace_fail("pg_alignment_trace", PG_E_BADARG, "mode must be 0 (global), 1 (local) or 2 (semi-global)");
  return trace_run("pg_alignment_trace", mode, x_packed, n, x_npad, xl, y_packed, m, y_npad, yl, xi, yi, npairs, table, gap,
                   gap_open, head, ops, ldo, workspace, workspace_bytes, stream);
}

// mode PG_TR_FIT: all of y within any substring of x (pg_aln_trace.h).  The entry above goes on rejecting mode 3.
int pg_alignment_fit_trace(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
    int64_t y_npad, int yl, const int32_t *xi, const int32_t *yi, int64_t npairs, const void *table, int gap, int gap_open,
    int32_t *head, uint8_t *ops, int64_t ldo, void *workspace, int64_t workspace_bytes, void *stream) {
  return trace_run("pg_alignment_fit_trace", PG_TR_FIT, x_packed, n, x_npad, xl, y_packed, m, y_npad, yl, xi, yi, npairs, table, gap,
                   gap_open, head, ops, ldo, workspace, workspace_bytes, stream);
}

}  // extern "C"
