// SEMI-GLOBAL ("overlap", end-gap-free) alignment score with Gotoh's affine gaps: both sequences are aligned end to end,
// the unaligned ends of either cost nothing.  Under a symmetric SCORE table S (larger is nearer), e = gap, o = gap_open:
//     H[i][0] = H[0][j] = 0,  E[0][j] = F[i][0] = -inf,
//     E[i][j] = max(E[i-1][j] - e, H[i-1][j] - o - e),   F[i][j] = max(F[i][j-1] - e, H[i][j-1] - o - e),
//     H[i][j] = max(H[i-1][j-1] + S[x_i][y_j], E[i][j], F[i][j])                                     (no zero floor),
//     s(y, x) = max(max over i of H[i][len y], max over j of H[len x][j]).
// BUILD DEFINED.  A similarity, >= 0 (H[0][len y] = 0).  Two kernels, pg_aln_semiglobal_dense_kernel up to 128 positions and
// pg_aln_semiglobal_long_dense_kernel up to 2048: the two frames of pg_aln_frame.h around the cell loop of pg_aln_score.h, with
// row 0 = Z, the masked last column folded at every step and row len x folded after the loop.
//
// Arithmetic.  Cells go negative, the registers are unsigned: a cell holds H + Z, E + Z, F + Z with the wave-uniform
// offset Z = min(xl, yl) * max(0, max S) of the operand WIDTHS, and every subtraction saturates as in pg_aln_local.hip
// (the profile holds S + bias, bias = -min S; the diagonal term is (H + byte) -sat- bias).  Saturation is therefore a
// floor at -Z, and the floor is exact: a cell whose stored value differs from the recurrence's is at most
// -Z + (what an alignment can still gain) <= -Z + min(len x, len y) * max S <= 0, by induction along any path that
// passes through a clamped cell, and 0 = H[0][len y] is in the result anyway.  The borders, -inf (E of row 0, F of
// column 0: stored 0) and the initial maximum are Z | 0 << 16; the result is best - Z.  A true H is at most
// min(i, j) * max S <= Z, so a stored one is at most 2 Z and the sum formed before the bias comes off at most
// 2 Z + 255: 32 767 at 128 * 127 (short kernel), and what the caller of the long entry guarantees to be <= 65 535.
//
// Where the result is read.  (1) Row len x: outer steps past a lane's own length run under the EXEC mask (`i < lx`), so
// after the outer loop the lane's column registers ARE row len x: one fold after the loop, nothing in it.  (2) Column
// len y: folded at every step i < lx; len y is wave-uniform but a run-time value inside the last chunk, so the 16 cells
// of that chunk are and-ed with 16 scalar masks (one of them all ones) before the fold - a stored value is unsigned,
// so a masked-out cell is 0 <= best.  An interior cell (j < len y, i < len x) is never folded.  (3) Padding: profile
// bytes at j >= len y are 0 (a score of -bias <= 0), so a padded cell is at most a last-column cell of the same or an
// earlier step - the fold after the loop may include them.
// The mode itself, AlnSemiglobal, is in pg_aln_score.h: pg_aln_profile.hip runs it on profiles.
#include "pg_aln_score.h"

template <typename OUT>
__global__ __launch_bounds__(ALN_THREADS) __attribute__((amdgpu_waves_per_eu(3))) void pg_aln_semiglobal_dense_kernel(
    const u32 *__restrict__ xt, long long n, long long xnpad, int xl, const u32 *__restrict__ yt, long long m, long long ynpad,
    int yl, const void *__restrict__ score, u32 gap, u32 open, int obias, OUT *__restrict__ out, long long ldo, long long colTiles) {
  aln_short_frame<AlnSemiglobal>(xt, n, xnpad, xl, yt, m, ynpad, yl, score, gap, open, obias, out, ldo, colTiles);
}

template <typename OUT>
__global__ __launch_bounds__(ALN_THREADS) void pg_aln_semiglobal_long_dense_kernel(
    const u32 *__restrict__ xt, long long n, long long xnpad, int xl, const u32 *__restrict__ yt, long long m, long long ynpad,
    int yl, const void *__restrict__ score, u32 gap, u32 open, int obias, OUT *__restrict__ out, long long ldo, int colTiles,
    int items, u32 *ws) {
  aln_long_frame<AlnSemiglobal>(xt, n, xnpad, xl, yt, m, ynpad, yl, score, gap, open, obias, out, ldo, colTiles, items, ws);
}

extern "C" {

int pg_alignment_semiglobal_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                                  int64_t y_npad, int yl, const int8_t *score_i8, int gap, int gap_open, void *out, int64_t ldo,
                                  int out_elem_bytes, void *stream) {
  const AlnCall c = {x_packed, n, x_npad, xl, y_packed, m, y_npad, yl, score_i8, gap, gap_open, 0, out, ldo, out_elem_bytes, nullptr, 0, stream};
  return aln_launch_short("pg_alignment_semiglobal_dense", c, pg_aln_semiglobal_dense_kernel<_Float16>,
                          pg_aln_semiglobal_dense_kernel<long long>);
}

int pg_alignment_semiglobal_long_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                                       int64_t y_npad, int yl, const int8_t *score_i8, int gap, int gap_open, void *out,
                                       int64_t ldo, int out_elem_bytes, void *workspace, int64_t workspace_bytes, void *stream) {
  const AlnCall c = {x_packed, n,   x_npad,         xl,        y_packed,        m,     y_npad, yl, score_i8, gap, gap_open, 0,
                     out,      ldo, out_elem_bytes, workspace, workspace_bytes, stream};
  return aln_launch_long("pg_alignment_semiglobal_long_dense", c, pg_aln_semiglobal_long_dense_kernel<int>,
                         pg_aln_semiglobal_long_dense_kernel<long long>);
}

}  // extern "C"
