// LOCAL alignment score (Smith-Waterman with Gotoh's affine gaps): the best score of any pair of substrings of the two
// sequences under a symmetric SCORE table S (larger is nearer) and gap penalties e = gap, o = gap_open.  A similarity,
// not a distance:
//     H[i][0] = H[0][j] = 0,  E[0][j] = F[i][0] = -inf,
//     E[i][j] = max(E[i-1][j] - e, H[i-1][j] - o - e),   F[i][j] = max(F[i][j-1] - e, H[i][j-1] - o - e),
//     H[i][j] = max(0, H[i-1][j-1] + S[x_i][y_j], E[i][j], F[i][j]),                  s(y, x) = max over i, j of H[i][j]
// BUILD DEFINED.  The frame is pg_aln_frame.h's, the cell loop pg_aln_score.h's with Z = 0, every cell folded into the
// maximum and no fold after the loop; the same mode serves pg_aln_long.hip's kernel beyond 128 positions.
//
// Arithmetic.  Everything is unsigned.  E and F are clamped at 0: a clamped value never beats the floor of H, so no H
// changes, and every subtraction is a saturating one (v_sub_u32 ... clamp; the pair H - o - e, E - e is one
// v_pk_sub_u16 ... clamp).  The profile holds S + bias, bias = -min(S over the 32 x 32 table) >= 0 (found here), so
// that its entries are bytes; the diagonal term is (H + byte) -sat- bias, which is max(0, H + S).  A cell is at most
// 128 * 127 = 16 256 and H + byte below 16 600, so H[j] and E[j] are the halves of one dword, P[j] = H | E << 16, as in
// pg_aln_affine.hip.  Per cell:  t = (diag + byte) -sat- bias;  E = max(E -sat- e, H -sat- (o + e));
// F = max(F -sat- e, left -sat- (o + e));  left = max3(t, E, F);  and once per two cells best = max3(best, h, h').
//
// What the global kernels need not do.  (1) Every cell is read - the result is the running maximum - so a cell that
// belongs to no pair of symbols must not raise it.  Positions j >= len y of a profile hold byte 0 (score -bias <= 0,
// whatever S[a][0] is): by induction such a cell is at most an H of a real cell of the same or an earlier outer step,
// which the maximum has seen, and cells of lower j never read it.  Outer steps past a lane's own length run under the
// EXEC mask (`i < lx`), the fold of the maximum with them.  (2) `best` is E-free: E and F are at most some earlier H.
#include "pg_aln_score.h"

template <typename OUT>
__global__ __launch_bounds__(ALN_THREADS) __attribute__((amdgpu_waves_per_eu(3))) void pg_aln_local_dense_kernel(
    const u32 *__restrict__ xt, long long n, long long xnpad, int xl, const u32 *__restrict__ yt, long long m, long long ynpad,
    int yl, const void *__restrict__ score, u32 gap, u32 open, int obias, OUT *__restrict__ out, long long ldo, long long colTiles) {
  aln_short_frame<AlnLocal>(xt, n, xnpad, xl, yt, m, ynpad, yl, score, gap, open, obias, out, ldo, colTiles);
}

extern "C" {

int pg_alignment_local_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                             int64_t y_npad, int yl, const int8_t *score_i8, int gap, int gap_open, void *out, int64_t ldo,
                             int out_elem_bytes, void *stream) {
  const AlnCall c = {x_packed, n, x_npad, xl, y_packed, m, y_npad, yl, score_i8, gap, gap_open, 0, out, ldo, out_elem_bytes, nullptr, 0, stream};
  return aln_launch_short("pg_alignment_local_dense", c, pg_aln_local_dense_kernel<_Float16>, pg_aln_local_dense_kernel<long long>);
}

}  // extern "C"
