// Alignment distances and local alignment scores of sequences BEYOND 128 positions (up to PG_ALN_LONG_MAX_L = 2048):
// the recurrences of pg_aln_affine.hip (global, Gotoh) and pg_aln_local.hip (Smith-Waterman, Gotoh), strip-mined along
// the Y side.  BUILD DEFINED.  One kernel template <MODE, OUT> on the long frame of pg_aln_frame.h; the global mode, below, is
// always in Gotoh form: gap_open = 0 is the linear gap penalty exactly (E = min(E + e, H + e)); the local mode is
// pg_aln_score.h's.  H | E << 16 in one register per cell, lanes past their own len x masked out.
//
// Strips.  The short kernels keep the DP column of the whole Y row in registers (P[16 * NC + 1], NC <= 8); nothing limits
// the X side, which the outer loop streams.  Here a Y row is cut into strips of ALN_STRIP = 128 positions, strip s the
// columns j0 + 1 .. j0 + 128, j0 = 128 s.  For every strip a wave initialises P[] to row 0 of the recurrence at the
// ABSOLUTE j (global: H[0][j] = o + j e, E[0][j] = H[0][j] + o standing for infinity; local: 0) and runs the whole outer
// loop over i.  Strips wholly beyond the row's len y are never run (the strip count is wave-uniform); every strip but
// the last runs NC = 8, the last one the compile-time switch on NC = ceil((len y - j0) / 16).
//
// The boundary column.  At outer step i the left edge of strip s > 0 is H[i][j0] and F[i][j0], which strip s - 1 wrote
// when it finished its step i: one dword H | F << 16 per (lane, i) in a global workspace laid out [i][thread], so a wave
// reads and writes one coalesced 256-byte line per step - one load and one store per ~1000 VALU instructions.  A lane
// reads back only what it wrote itself (the same thread, the same address), so no other wave's stores are ever
// consumed.  The step's diagonal H[i-1][j0] is the H loaded by the previous step (P[0]).  Strip 0 starts from column 0 as
// the short kernels do: H[i][0] = o + i e, F[i][0] = H[i][0] + o (global); 0 (local).  Masked steps (i >= len x of the
// lane) neither read nor write the workspace.
//
// Workspace.  Caller-owned (pg_alignment_long_workspace), sized per workgroup IN FLIGHT, not per tile of the problem:
// 256 * xl_padded * 4 bytes each, xl_padded = xl rounded up to 4.  The entry launches at most as many workgroups as the
// workspace holds; workgroup b owns slice b and loops over its (column tile, row group) items.
//
// LDS.  A workgroup works on one Y row at a time (the workspace holds one boundary column per lane) and uses the
// ALN_ROWS = 8 profile slots of the short kernels for up to 8 consecutive STRIPS of that row: one build and one barrier
// per 1024 positions.  36 KiB of profiles, the row's tokens (2 KiB), the staged table.
//
// 16-bit cells.  Global: a cell is at most W * max(max C, e) + o, W = max(xl, yl) (align the shorter sequence, gap the
// rest in one run); E and F are at most one o + e above an H, and the sums formed before a min add e once more:
//     W * max(max C, e) + 2 o + 2 e <= 65 535
// is what the caller guarantees (cells right of len y inside the last strip may wrap: nothing left of them reads them).
// Local: a cell is at most min(xl, yl) * max(S) and the diagonal term adds a profile byte (S + bias <= 255):
//     min(xl, yl) * max(S) + 255 <= 65 535.
// The kernel does not test either.
//
// Local scores across strips (the two rules of pg_aln_local.hip): profile bytes at ABSOLUTE positions j >= len y are 0,
// and the fold of the running maximum - carried in a register from strip to strip - sits inside `i < lx`, so a boundary
// column is never read, and nothing folded, past a lane's len x.
#include "pg_aln_score.h"

// One strip of one Y row against the lane's X sequence, global alignment.  Q: the strip's profile; j0: its first column - 1;
// jl: the local index of len y in the last strip (else 0); carry_out: write the boundary column for the next strip.
// Returns H[lx][len y] (last strip).
template <int NC>
__device__ __forceinline__ u32 alng_strip(const unsigned char *Q, const AlnX &x, u32 *wsb, int j0, int jl, bool carry_out, u32 e, u32 o) {
  const u32 oe = o + e, K = oe | (e << 16);
  u32 P[16 * NC + 1];                                                     // P[j] = H[j0 + j] | E[j0 + j] << 16; P[0]: H alone
  const u32 b = o + (u32)j0 * e;                                          // H[0][j0], j0 > 0
  P[0] = j0 ? b : 0u;
#pragma unroll
  for (int j = 1; j <= 16 * NC; ++j) P[j] = (b + (u32)j * e) | ((b + o + (u32)j * e) << 16);
  u32 xw = 0, h0 = o;
  for (int i = 0; i < x.lxmax; ++i) {
    if ((i & 3) == 0) xw = aln_x_word(x, i);
    const u32 a = (xw >> (8 * (i & 3))) & 31u;
    h0 += e;                                                              // H[i + 1][0] = o + (i + 1) e
    if (i < x.lx) {
      const unsigned char *q = Q + a * ALN_QSTRIDE;
      u32 *bd = wsb + (long long)i * ALN_THREADS;                         // this step's line of the boundary column
      u32 left, F;
      if (j0) {                                                           // wave-uniform
        const u32 v = bd[x.lane];
        left = v & 0xffffu;
        F = v >> 16;
      } else {
        left = h0;
        F = h0 + o;                                                       // F[i][0]: what infinity would give
      }
      u32 diag = P[0];
      P[0] = left;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const uint4 v = *(const uint4 *)(q + 16 * c);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
        // the diagonal terms first, from the old column: afterwards every cell is rewritten in place
        u32 T[16];
        T[0] = (diag & 0xffffu) + (w[0] & 255u);
#pragma unroll
        for (int t = 1; t < 16; ++t) T[t] = (P[16 * c + t] & 0xffffu) + ((w[t >> 2] >> (8 * (t & 3))) & 255u);
        diag = P[16 * c + 16];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const u32 s = P[16 * c + t + 1] + K;                            // H + o + e | (E + e) << 16
          const u32 E = min(s & 0xffffu, s >> 16);
          F = min(F + e, left + oe);
          left = min(T[t], min(E, F));
          P[16 * c + t + 1] = left | (E << 16);
        }
      }
      if (carry_out) bd[x.lane] = left | (F << 16);                       // H[i + 1][j0 + 128] | F[i + 1][j0 + 128] << 16
    }
  }
  u32 res = 0;                                                            // H[len y], 16 (NC - 1) < jl <= 16 NC, jl wave-uniform
#pragma unroll
  for (int t = 1; t <= 16; ++t)
    if (jl == 16 * (NC - 1) + t) res = P[16 * (NC - 1) + t];
  return res & 0xffffu;
}

struct AlnGlobalLong : AlnModeBase {
  static constexpr bool SCORE = false, TOP = false;
  u32 gap, open;
  __device__ __forceinline__ AlnGlobalLong(const AlnParams &p) : gap(p.gap), open(p.open) {}
  __device__ __forceinline__ u32 first(int, int lx) const { return lx ? open + (u32)lx * gap : 0u; }      // len y = 0: one run of lx symbols, or nothing
  template <int NC, bool LAST>
  __device__ __forceinline__ u32 strip(const unsigned char *q, const AlnX &x, u32 *wsb, int j0, int rest, u32) const {
    return alng_strip<NC>(q, x, wsb, j0, rest, !LAST, gap, open);
  }
};

// pg_aln_list_long.hip includes this file for the mode above alone (its list instance needs AlnGlobalLong, which lives here)
#ifndef ALN_LONG_MODE_ONLY
template <class MODE, typename OUT>
__global__ __launch_bounds__(ALN_THREADS) void pg_aln_long_dense_kernel(
    const u32 *__restrict__ xt, long long n, long long xnpad, int xl, const u32 *__restrict__ yt, long long m, long long ynpad,
    int yl, const void *__restrict__ table, u32 gap, u32 open, int obias, OUT *__restrict__ out, long long ldo, int colTiles,
    int items, u32 *ws) {
  aln_long_frame<MODE>(xt, n, xnpad, xl, yt, m, ynpad, yl, table, gap, open, obias, out, ldo, colTiles, items, ws);
}

extern "C" {

int pg_alignment_long_workspace(int xl, int64_t *one_workgroup_bytes, int64_t *full_bytes) {
  if (xl <= 0 || (!one_workgroup_bytes && !full_bytes)) return pg_fail(PG_E_BADARG, "pg_alignment_long_workspace: bad argument");
  if (xl > ALNG_MAX_L) return pg_fail(PG_E_TOOLONG, "pg_alignment_long_workspace: at most 2048 positions");
  const int64_t one = aln_long_share(xl);
  if (one_workgroup_bytes) *one_workgroup_bytes = one;
  if (full_bytes) {
    int dev = 0;
    hipDeviceProp_t prop;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, dev);
    if (e != hipSuccess) return pg_launched((int)e, "pg_alignment_long_workspace");
    *full_bytes = one * prop.multiProcessorCount * ALNG_RESIDENT;
  }
  return 0;
}

int pg_alignment_long_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                            int64_t y_npad, int yl, const uint8_t *cost_u8, int gap, int gap_open, void *out, int64_t ldo,
                            int out_elem_bytes, void *workspace, int64_t workspace_bytes, void *stream) {
  const AlnCall c = {x_packed, n,   x_npad,         xl,        y_packed,        m,     y_npad, yl, cost_u8, gap, gap_open, 0,
                     out,      ldo, out_elem_bytes, workspace, workspace_bytes, stream};
  return aln_launch_long("pg_alignment_long_dense", c, pg_aln_long_dense_kernel<AlnGlobalLong, int>,
                         pg_aln_long_dense_kernel<AlnGlobalLong, long long>);
}

int pg_alignment_local_long_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                                  int64_t y_npad, int yl, const int8_t *score_i8, int gap, int gap_open, void *out, int64_t ldo,
                                  int out_elem_bytes, void *workspace, int64_t workspace_bytes, void *stream) {
  const AlnCall c = {x_packed, n,   x_npad,         xl,        y_packed,        m,     y_npad, yl, score_i8, gap, gap_open, 0,
                     out,      ldo, out_elem_bytes, workspace, workspace_bytes, stream};
  return aln_launch_long("pg_alignment_local_long_dense", c, pg_aln_long_dense_kernel<AlnLocal, int>,
                         pg_aln_long_dense_kernel<AlnLocal, long long>);
}

}  // extern "C"
#endif  // ALN_LONG_MODE_ONLY
