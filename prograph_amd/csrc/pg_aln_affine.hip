// Gapped alignment distance with AFFINE gap penalties (global alignment, Gotoh's three-matrix recurrence): a maximal
// run of g unaligned symbols of one sequence costs gap_open + g * gap.  With e = gap, o = gap_open:
//     H[0][0] = 0,  H[0][j] = o + j e,  H[i][0] = o + i e,
//     E[i][j] = min(E[i-1][j] + e, H[i-1][j] + o + e)        run ending in a gap against x_i  (E[0][j] = inf)
//     F[i][j] = min(F[i][j-1] + e, H[i][j-1] + o + e)        run ending in a gap against y_j  (F[i][0] = inf)
//     H[i][j] = min(H[i-1][j-1] + C[x_i][y_j], E[i][j], F[i][j]),                              d(y, x) = H[lx][ly]
// BUILD DEFINED, as the linear form in pg_aln.hip, whose shape this kernel keeps (the frame: pg_aln_frame.h): lanes past
// their own length masked out, H[ly] picked by wave-uniform selects.
//
// State.  Across outer steps (one X symbol each) a lane keeps H[j] and E[j] for every j; F is a running scalar along j
// inside a step.  No infinity is stored: E[0][j] = H[0][j] + o and F[i][0] = H[i][0] + o make the first
// min(E + e, H + o + e) and min(F + e, H + o + e) return their second argument, which is what infinity would do.
// Every value fits 16 bits without a sign: H <= 128 * 255 + 2 * 255 and E, F <= H + 510, and the largest sum formed
// before a min adds 510 once more: below 35 000.
//
// Layouts (ALN_AFFINE_LAYOUT, chosen from the compiler's report and the ISA: profiles/aln_affine_dense.txt):
//     0  H[j] and E[j] as the two halves of one dword, P[j] = H | E << 16.  One 32-bit add of (o + e) | e << 16 forms
//        H + o + e and E + e at once (no carry crosses the halves: the sums stay below 65 536), the new E is the
//        min of the two halves, the new cell is repacked.
//     1  H and E as two 32-bit arrays, at every NC.
//     2  two 32-bit arrays while NC <= ALN_AFFINE_SPLIT, the packed form above that.
// Per cell:  t = diag + cost;  E = min(E + e, H + o + e);  F = min(F + e, left + o + e);  left = min3(t, E, F).
#include "pg_aln_frame.h"

#ifndef ALN_AFFINE_LAYOUT
#define ALN_AFFINE_LAYOUT 0
#endif
#ifndef ALN_AFFINE_SPLIT
#define ALN_AFFINE_SPLIT 4
#endif

// H and E as halves of one dword
template <int NC>
__device__ __forceinline__ u32 alna_row_packed(const unsigned char *Q, const AlnX &x, int ly, u32 e, u32 o) {
  const u32 oe = o + e, K = oe | (e << 16);
  u32 P[16 * NC + 1];
  P[0] = 0;
#pragma unroll
  for (int j = 1; j <= 16 * NC; ++j) P[j] = (o + (u32)j * e) | ((2 * o + (u32)j * e) << 16);
  u32 xw = 0, h0 = o;
  for (int i = 0; i < x.lxmax; ++i) {
    if ((i & 3) == 0) xw = aln_x_word(x, i);
    const u32 a = (xw >> (8 * (i & 3))) & 31u;
    h0 += e;                                                              // H[i + 1][0] = o + (i + 1) e
    if (i < x.lx) {
      const unsigned char *q = Q + a * ALN_QSTRIDE;
      u32 diag = P[0];
      u32 left = h0;
      u32 F = left + o;
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
    }
  }
  u32 res = 0;                                                            // H[ly], 16 (NC - 1) < ly <= 16 NC, ly wave-uniform
#pragma unroll
  for (int t = 1; t <= 16; ++t)
    if (ly == 16 * (NC - 1) + t) res = P[16 * (NC - 1) + t];
  return res & 0xffffu;
}

// H and E as two 32-bit arrays
template <int NC>
__device__ __forceinline__ u32 alna_row_wide(const unsigned char *Q, const AlnX &x, int ly, u32 e, u32 o) {
  const u32 oe = o + e;
  u32 H[16 * NC + 1], E[16 * NC + 1];
  H[0] = 0;
  E[0] = 0;
#pragma unroll
  for (int j = 1; j <= 16 * NC; ++j) {
    H[j] = o + (u32)j * e;
    E[j] = H[j] + o;
  }
  u32 xw = 0, h0 = o;
  for (int i = 0; i < x.lxmax; ++i) {
    if ((i & 3) == 0) xw = aln_x_word(x, i);
    const u32 a = (xw >> (8 * (i & 3))) & 31u;
    h0 += e;
    if (i < x.lx) {
      const unsigned char *q = Q + a * ALN_QSTRIDE;
      u32 diag = H[0];
      u32 left = h0;
      u32 F = left + o;
      H[0] = left;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const uint4 v = *(const uint4 *)(q + 16 * c);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
        u32 T[16];
        T[0] = diag + (w[0] & 255u);
#pragma unroll
        for (int t = 1; t < 16; ++t) T[t] = H[16 * c + t] + ((w[t >> 2] >> (8 * (t & 3))) & 255u);
        diag = H[16 * c + 16];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const u32 En = min(E[16 * c + t + 1] + e, H[16 * c + t + 1] + oe);
          F = min(F + e, left + oe);
          left = min(T[t], min(En, F));
          H[16 * c + t + 1] = left;
          E[16 * c + t + 1] = En;
        }
      }
    }
  }
  u32 res = 0;
#pragma unroll
  for (int t = 1; t <= 16; ++t)
    if (ly == 16 * (NC - 1) + t) res = H[16 * (NC - 1) + t];
  return res;
}

template <int NC>
__device__ __forceinline__ u32 alna_row(const unsigned char *Q, const AlnX &x, int ly, u32 e, u32 o) {
  if (ALN_AFFINE_LAYOUT == 1 || (ALN_AFFINE_LAYOUT == 2 && NC <= ALN_AFFINE_SPLIT))
    return alna_row_wide<NC>(Q, x, ly, e, o);
  return alna_row_packed<NC>(Q, x, ly, e, o);
}

struct AlnAffine : AlnModeBase {
  static constexpr bool SCORE = false, TOP = false;
  u32 gap, open;
  __device__ __forceinline__ AlnAffine(const AlnParams &p) : gap(p.gap), open(p.open) {}
  __device__ __forceinline__ u32 first(int, int lx) const { return lx ? open + (u32)lx * gap : 0u; }      // one run of lx symbols, or nothing
  template <int NC>
  __device__ __forceinline__ u32 row(const unsigned char *q, const AlnX &x, int ly) const { return alna_row<NC>(q, x, ly, gap, open); }
};

// pg_aln_list.hip includes this file for the mode above alone (its list instance needs AlnAffine, which lives here)
#ifndef ALN_AFFINE_MODE_ONLY
template <typename OUT>
__global__ __launch_bounds__(ALN_THREADS) void pg_aln_affine_dense_kernel(const u32 *__restrict__ xt, long long n, long long xnpad,
                                                                          int xl, const u32 *__restrict__ yt, long long m,
                                                                          long long ynpad, int yl, const void *__restrict__ cost,
                                                                          u32 gap, u32 open, int obias, OUT *__restrict__ out,
                                                                          long long ldo, long long colTiles) {
  aln_short_frame<AlnAffine>(xt, n, xnpad, xl, yt, m, ynpad, yl, cost, gap, open, obias, out, ldo, colTiles);
}

extern "C" {

int pg_alignment_affine_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                              int64_t y_npad, int yl, const uint8_t *cost_u8, int gap, int gap_open, void *out, int64_t ldo,
                              int out_elem_bytes, void *stream) {
  const AlnCall c = {x_packed, n, x_npad, xl, y_packed, m, y_npad, yl, cost_u8, gap, gap_open, 0, out, ldo, out_elem_bytes, nullptr, 0, stream};
  return aln_launch_short("pg_alignment_affine_dense", c, pg_aln_affine_dense_kernel<_Float16>, pg_aln_affine_dense_kernel<long long>);
}

}  // extern "C"
#endif
