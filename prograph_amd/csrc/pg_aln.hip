// Gapped alignment distance of tokenised sequences (global alignment, Needleman-Wunsch, linear gap penalty):
//     H[0][j] = j * gap,  H[i][0] = i * gap,
//     H[i][j] = min(H[i-1][j-1] + C[x_i][y_j], H[i-1][j] + gap, H[i][j-1] + gap),        d(y, x) = H[lx][ly]
// with a symmetric cost table C of at most 32 symbols, entries 0..255, and gap 1..255 (BUILD DEFINED: the reference has
// no such distance).  A row's sequence is the row without its trailing zeros; an interior zero is symbol 0 of C.
//
// One X sequence per lane, the Y row wave-uniform.  A workgroup of ALN_THREADS columns owns ALN_ROWS rows of Y and
// builds their query profiles in LDS once:
//     Q[r][a][j] = C[a][y_{r,j}]        one byte per (row r, symbol a, position j), ALN_QSTRIDE bytes per symbol
// A lane walks its own sequence in the outer loop; for its symbol x_i ONE 16-byte LDS read returns the costs of 16
// consecutive cells of the DP column, which lives in registers, H[0..16 * NC], indexed at compile time only: the
// kernel switches on the wave-uniform chunk count NC = ceil(ly / 16) per Y row.  Cells past ly inside the last chunk
// are computed and never read: a cell depends on cells at lower j only.  Per cell
//     t = diag + cost (the byte picked by the add itself);  u = up + gap;  v = left + gap;  left = min3(t, u, v)
// in 32-bit registers (a cell is at most 128 * 255 = 32 640).  Lanes whose sequences are shorter than the longest
// of their wave sit out the remaining outer steps (EXEC mask), so every lane ends with its own last DP row.
//
// ALN_QSTRIDE = 144: the 16-byte slot of a read is (9 a + chunk) mod 16, so the lanes of one ds_read_b128 group fall
// on different slots unless their symbols differ by 16; equal symbols broadcast.  A stride of 128 would put every
// symbol on one of two slots.
//
// Operands: the transposed dword order of pg_sub_pack (dword g of sequence c at (g * npad + c) * 4), so the 64 lanes
// of a wave load 64 consecutive columns coalesced.  Staging, lengths, the switch on NC and the host side: pg_aln_frame.h.
#include "pg_aln_frame.h"

template <int NC>
__device__ __forceinline__ u32 aln_row(const unsigned char *Q, const AlnX &x, int ly, u32 gap) {
  u32 H[16 * NC + 1];
#pragma unroll
  for (int j = 0; j <= 16 * NC; ++j) H[j] = (u32)j * gap;
  u32 xw = 0;
  for (int i = 0; i < x.lxmax; ++i) {
    if ((i & 3) == 0) xw = aln_x_word(x, i);
    const u32 a = (xw >> (8 * (i & 3))) & 31u;
    if (i < x.lx) {
      const unsigned char *q = Q + a * ALN_QSTRIDE;
      u32 diag = H[0];
      u32 left = diag + gap;
      H[0] = left;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const uint4 v = *(const uint4 *)(q + 16 * c);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
        // the diagonal terms first, from the old column: afterwards every cell is rewritten in place and no old
        // value has to be kept in a second register
        u32 T[16];
        T[0] = diag + (w[0] & 255u);
#pragma unroll
        for (int t = 1; t < 16; ++t) T[t] = H[16 * c + t] + ((w[t >> 2] >> (8 * (t & 3))) & 255u);
        diag = H[16 * c + 16];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          left = min(T[t], min(H[16 * c + t + 1] + gap, left + gap));
          H[16 * c + t + 1] = left;
        }
      }
    }
  }
  u32 res = 0;                                                            // H[ly], 16 (NC - 1) < ly <= 16 NC, ly wave-uniform
#pragma unroll
  for (int t = 1; t <= 16; ++t)
    if (ly == 16 * (NC - 1) + t) res = H[16 * (NC - 1) + t];
  return res;
}

struct AlnLinear : AlnModeBase {
  static constexpr bool SCORE = false, TOP = false;
  u32 gap;
  __device__ __forceinline__ AlnLinear(const AlnParams &p) : gap(p.gap) {}
  __device__ __forceinline__ u32 first(int, int lx) const { return (u32)lx * gap; }
  template <int NC>
  __device__ __forceinline__ u32 row(const unsigned char *q, const AlnX &x, int ly) const { return aln_row<NC>(q, x, ly, gap); }
};

template <typename OUT>
__global__ __launch_bounds__(ALN_THREADS) void pg_aln_dense_kernel(const u32 *__restrict__ xt, long long n, long long xnpad, int xl,
                                                                   const u32 *__restrict__ yt, long long m, long long ynpad, int yl,
                                                                   const void *__restrict__ cost, u32 gap, u32 open, int obias,
                                                                   OUT *__restrict__ out, long long ldo, long long colTiles) {
  aln_short_frame<AlnLinear>(xt, n, xnpad, xl, yt, m, ynpad, yl, cost, gap, open, obias, out, ldo, colTiles);
}

extern "C" {

int pg_alignment_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m, int64_t y_npad,
                       int yl, const uint8_t *cost_u8, int gap, void *out, int64_t ldo, int out_elem_bytes, void *stream) {
  const AlnCall c = {x_packed, n, x_npad, xl, y_packed, m, y_npad, yl, cost_u8, gap, 0, 0, out, ldo, out_elem_bytes, nullptr, 0, stream};
  return aln_launch_short("pg_alignment_dense", c, pg_aln_dense_kernel<_Float16>, pg_aln_dense_kernel<long long>);
}

}  // extern "C"
