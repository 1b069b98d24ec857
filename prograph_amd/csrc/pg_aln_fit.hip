// FIT ("glocal") alignment score with Gotoh's affine gaps: ALL of y is aligned, within ANY substring of x - only the ends of
// x are free.  Under a symmetric SCORE table S (larger is nearer), e = gap, o = gap_open, i over x and j over y:
//     H[i][0] = 0,  H[0][j] = -(o + j e) (j >= 1),  E[0][j] = F[i][0] = -inf,
//     E[i][j] = max(E[i-1][j] - e, H[i-1][j] - o - e),   F[i][j] = max(F[i][j-1] - e, H[i][j-1] - o - e),
//     H[i][j] = max(H[i-1][j-1] + S[x_i][y_j], E[i][j], F[i][j])                                     (no zero floor),
//     s(y, x) = max over i = 0..len x of H[i][len y].
// BUILD DEFINED.  A similarity, NOT symmetric, and it may be negative: -(o + e len y) <= s <= min(len x, len y) max S.
// Two kernels, pg_aln_fit_dense_kernel up to 128 positions and pg_aln_fit_long_dense_kernel up to 2048: the two frames of
// pg_aln_frame.h around the cell loop of pg_aln_score.h, with row 0 the chain -(o + j e), the masked last column folded at
// every step and NO fold after the loop.
//
// Arithmetic.  The registers are unsigned: a cell holds H + Z, E + Z, F + Z with the wave-uniform offset
//     Z = o + yl (e + top),   top = max(0, max S),   yl = the WIDTH of the Y operand (len y <= yl),
// and every subtraction saturates (the profile holds S + bias, bias = -min S; the diagonal term is (H + byte) -sat- bias).
// Saturation is a floor at -Z, -inf is stored as 0 = -Z, and the floor is exact: by induction along any path that passes
// through a cell whose stored value differs from the recurrence's, the H[i][len y] it reaches is at most
//     -Z + (what the rest of y can still gain) <= -Z + len y * top <= -(o + e yl) <= -(o + e len y) = H[0][len y],
// and H[0][len y] is in the result anyway.  The borders of row 0 are Z - (o + j e) >= 0 for j <= yl (columns of the last
// chunk past yl saturate; they are padding, see (3)).  A true H[i][j] is at most j top <= yl top, so a stored one is at
// most Z + yl top and the sum formed before the bias comes off at most
//     o + yl (e + 2 top) + 255 <= 65 535,
// which the caller of EITHER entry guarantees (128 positions at 255 / 255 / 127 give 65 662: the short kernel needs the
// predicate too).  The result is best - Z + out_bias as a signed number; out_bias >= 0 is the caller's shift for the
// selection layers, which sort non-negative values.
//
// Where the result is read.  (1) The initial maximum is H[0][len y] = Z - (o + e len y), Z for an empty y.  (2) Column
// len y: folded at every step i < lx; len y is wave-uniform but a run-time value inside the last chunk, so the 16 cells of
// that chunk are and-ed with 16 scalar masks (one of them all ones) before the fold - a stored value is unsigned, so a
// masked-out cell is 0 <= best.  Nothing else is folded: no interior cell, and NOT row len x.  (3) Padding: a cell reads
// cells of lower or equal j only, so the cells j > len y of the last chunk feed no cell j <= len y; they are never folded,
// and the boundary column is written by strips that lie wholly inside len y.  A lane past its own len x keeps its cells
// under the EXEC mask (`i < lx`).
// The mode itself, AlnFit, is in pg_aln_score.h: pg_aln_profile.hip runs it on profiles.
#include "pg_aln_score.h"

template <typename OUT>
__global__ __launch_bounds__(ALN_THREADS) __attribute__((amdgpu_waves_per_eu(3))) void pg_aln_fit_dense_kernel(
    const u32 *__restrict__ xt, long long n, long long xnpad, int xl, const u32 *__restrict__ yt, long long m, long long ynpad,
    int yl, const void *__restrict__ score, u32 gap, u32 open, int obias, OUT *__restrict__ out, long long ldo, long long colTiles) {
  aln_short_frame<AlnFit>(xt, n, xnpad, xl, yt, m, ynpad, yl, score, gap, open, obias, out, ldo, colTiles);
}

template <typename OUT>
__global__ __launch_bounds__(ALN_THREADS) void pg_aln_fit_long_dense_kernel(
    const u32 *__restrict__ xt, long long n, long long xnpad, int xl, const u32 *__restrict__ yt, long long m, long long ynpad,
    int yl, const void *__restrict__ score, u32 gap, u32 open, int obias, OUT *__restrict__ out, long long ldo, int colTiles,
    int items, u32 *ws) {
  aln_long_frame<AlnFit>(xt, n, xnpad, xl, yt, m, ynpad, yl, score, gap, open, obias, out, ldo, colTiles, items, ws);
}

extern "C" {

int pg_alignment_fit_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                           int64_t y_npad, int yl, const int8_t *score_i8, int gap, int gap_open, int bias, void *out,
                           int64_t ldo, int out_elem_bytes, void *stream) {
  const AlnCall c = {x_packed, n, x_npad, xl, y_packed, m, y_npad, yl, score_i8, gap, gap_open, bias, out, ldo, out_elem_bytes, nullptr, 0, stream};
  return aln_launch_short("pg_alignment_fit_dense", c, pg_aln_fit_dense_kernel<_Float16>, pg_aln_fit_dense_kernel<long long>);
}

int pg_alignment_fit_long_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                                int64_t y_npad, int yl, const int8_t *score_i8, int gap, int gap_open, int bias, void *out,
                                int64_t ldo, int out_elem_bytes, void *workspace, int64_t workspace_bytes, void *stream) {
  const AlnCall c = {x_packed, n,   x_npad,         xl,        y_packed,        m,     y_npad, yl, score_i8, gap, gap_open, bias,
                     out,      ldo, out_elem_bytes, workspace, workspace_bytes, stream};
  return aln_launch_long("pg_alignment_fit_long_dense", c, pg_aln_fit_long_dense_kernel<int>, pg_aln_fit_long_dense_kernel<long long>);
}

}  // extern "C"
