// LOCAL alignment score (Smith-Waterman with Gotoh's affine gaps): the best score of any pair of substrings of the two
// sequences under a symmetric SCORE table S (larger is nearer) and gap penalties e = gap, o = gap_open.  A similarity,
// not a distance:
//     H[i][0] = H[0][j] = 0,  E[0][j] = F[i][0] = -inf,
//     E[i][j] = max(E[i-1][j] - e, H[i-1][j] - o - e),   F[i][j] = max(F[i][j-1] - e, H[i][j-1] - o - e),
//     H[i][j] = max(0, H[i-1][j-1] + S[x_i][y_j], E[i][j], F[i][j]),                  s(y, x) = max over i, j of H[i][j]
// BUILD DEFINED.  The shape of pg_aln_affine.hip: one X sequence per lane, ALN_ROWS wave-uniform Y rows per workgroup,
// their query profiles Q[r][a][j] in LDS at stride ALN_QSTRIDE, one 16-byte LDS read per 16 cells, a compile-time switch
// on NC = ceil(ly / 16), the lengths found here, lanes past their own length masked out.  The staging code below is that
// kernel's, repeated here so that pg_aln.hip and pg_aln_affine.hip stay as they are.
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
#include "pg_common.h"
#include "../../include/prograph_hip.h"

#define ALN_THREADS 256
#define ALN_ROWS 8                 // Y rows per workgroup: 8 profiles = 36 KiB of LDS
#define ALN_MAX_L 128
#define ALN_QSTRIDE 144
#define ALN_QBYTES (32 * ALN_QSTRIDE)
#define ALN_CSTRIDE 36             // bytes per row of the staged score table (as in pg_sub.hip)

typedef unsigned short alnl_u16x2 __attribute__((ext_vector_type(2)));

// index of the last non-zero byte + 1 over the dwords of one sequence, 0 for an empty one
__device__ __forceinline__ int alnl_len_step(int len, u32 w, int g) { return w ? 4 * g + 4 - (__clz(w) >> 3) : len; }

// a - b, 0 where b > a
__device__ __forceinline__ u32 alnl_sat(u32 a, u32 b) { return __builtin_elementwise_sub_sat(a, b); }

// the same on both 16-bit halves at once
__device__ __forceinline__ u32 alnl_sat2(u32 a, u32 b) {
  return __builtin_bit_cast(u32, __builtin_elementwise_sub_sat(__builtin_bit_cast(alnl_u16x2, a), __builtin_bit_cast(alnl_u16x2, b)));
}

template <int NC>
__device__ __forceinline__ u32 alnl_row(const unsigned char *Q, const u32 *xb, int lane, long long xnpad, int lx, int lxmax, u32 e,
                                        u32 oe, u32 bias) {
  const u32 K = oe | (e << 16);
  u32 P[16 * NC + 1];                                                     // P[j] = H[j] | E[j] << 16; P[0] stays 0
#pragma unroll
  for (int j = 0; j <= 16 * NC; ++j) P[j] = 0;
  u32 xw = 0, best = 0;
  for (int i = 0; i < lxmax; ++i) {
    if ((i & 3) == 0) xw = (xb + (long long)(i >> 2) * xnpad)[lane];          // wave-uniform branch and base, coalesced load
    const u32 x = (xw >> (8 * (i & 3))) & 31u;
    if (i < lx) {
      const unsigned char *q = Q + x * ALN_QSTRIDE;
      u32 diag = 0, left = 0, F = 0;                                      // H[i][0] = 0, F[i][0] = -inf clamped
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const uint4 v = *(const uint4 *)(q + 16 * c);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
        // the diagonal terms first, from the old column: afterwards every cell is rewritten in place
        u32 T[16];
        T[0] = alnl_sat((diag & 0xffffu) + (w[0] & 255u), bias);
#pragma unroll
        for (int t = 1; t < 16; ++t) T[t] = alnl_sat((P[16 * c + t] & 0xffffu) + ((w[t >> 2] >> (8 * (t & 3))) & 255u), bias);
        diag = P[16 * c + 16];
#pragma unroll
        for (int t = 0; t < 16; t += 2) {
          u32 h[2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const u32 s = alnl_sat2(P[16 * c + t + u + 1], K);            // H -sat- (o + e) | (E -sat- e) << 16
            const u32 E = max(s & 0xffffu, s >> 16);
            F = max(alnl_sat(F, e), alnl_sat(left, oe));
            left = max(T[t + u], max(E, F));
            P[16 * c + t + u + 1] = left | (E << 16);
            h[u] = left;
          }
          best = max(max(best, h[0]), h[1]);
        }
      }
    }
  }
  return best;
}

template <typename OUT>
__global__ __launch_bounds__(ALN_THREADS) __attribute__((amdgpu_waves_per_eu(3))) void pg_aln_local_dense_kernel(
    const u32 *__restrict__ xt, long long n, long long xnpad, int xl, const u32 *__restrict__ yt, long long m, long long ynpad,
    int yl, const signed char *__restrict__ score, u32 gap, u32 open, OUT *__restrict__ out, long long ldo, long long colTiles) {
  __shared__ __attribute__((aligned(16))) unsigned char Q[ALN_ROWS * ALN_QBYTES];
  __shared__ u32 ytile[ALN_ROWS][ALN_MAX_L / 4];
  __shared__ unsigned char cs[32 * ALN_CSTRIDE];
  __shared__ int ylen[ALN_ROWS];
  __shared__ int smin;
  const int tid = threadIdx.x;
  const long long ct = (long long)blockIdx.x % colTiles, rg = (long long)blockIdx.x / colTiles;
  const long long row0 = rg * ALN_ROWS;
  const int xg = (xl + 3) >> 2, yg = (yl + 3) >> 2;                         // <= 32 dwords each (the host checks)

  if (tid == 0) smin = 0;
  for (int i = tid; i < ALN_ROWS * (ALN_MAX_L / 4); i += ALN_THREADS) {
    const int r = i >> 5, g = i & 31;
    ytile[r][g] = (row0 + r < m && g < yg) ? yt[(long long)g * ynpad + row0 + r] : 0u;
  }
  int sc[4], lo = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    sc[k] = score[tid + k * ALN_THREADS];
    lo = min(lo, sc[k]);
  }
  __syncthreads();
  if (lo < 0) atomicMin(&smin, lo);
  if (tid < ALN_ROWS) {
    int len = 0;
    for (int g = 0; g < ALN_MAX_L / 4; ++g) len = alnl_len_step(len, ytile[tid][g], g);
    ylen[tid] = len;
  }
  __syncthreads();
  const u32 bias = (u32)(-__builtin_amdgcn_readfirstlane(smin));             // 0..128, in a scalar register
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = tid + k * ALN_THREADS;
    cs[(i >> 5) * ALN_CSTRIDE + (i & 31)] = (unsigned char)(sc[k] + (int)bias);
  }
  __syncthreads();
  for (int i = tid; i < ALN_ROWS * 32 * 32; i += ALN_THREADS) {
    const int g = i & 31, a = (i >> 5) & 31, r = i >> 10;
    const u32 w = ytile[r][g];
    const unsigned char *crow = cs + a * ALN_CSTRIDE;                       // S is symmetric: S[a][y] = S[y][a]
    const u32 d = (u32)crow[w & 31u] | ((u32)crow[(w >> 8) & 31u] << 8) | ((u32)crow[(w >> 16) & 31u] << 16) |
                  ((u32)crow[(w >> 24) & 31u] << 24);
    const int keep = ylen[r] - 4 * g;                                       // positions of this dword inside the sequence
    const u32 mask = keep >= 4 ? 0xffffffffu : keep <= 0 ? 0u : (1u << (8 * keep)) - 1u;
    *(u32 *)(Q + r * ALN_QBYTES + a * ALN_QSTRIDE + 4 * g) = d & mask;      // past len y: byte 0, a score of -bias
  }
  __syncthreads();

  // column ct * 256 + tid (< colTiles * 256 <= xnpad): a wave-uniform base and the lane, so that one VGPR addresses both
  // the tokens and the output
  const u32 *xb = xt + ct * ALN_THREADS;
  const long long left_cols = n - ct * ALN_THREADS;                         // >= 1
  int lx = 0;
  for (int g = 0; g < xg; ++g) lx = alnl_len_step(lx, (xb + (long long)g * xnpad)[tid], g);
  if (tid >= left_cols) lx = 0;
  int lxmax = lx;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) lxmax = max(lxmax, __shfl_xor(lxmax, s));
  lxmax = __builtin_amdgcn_readfirstlane(lxmax);

  const u32 oe = open + gap;
  for (int r = 0; r < ALN_ROWS; ++r) {
    const long long row = row0 + r;
    if (row >= m) break;
    const int ly = __builtin_amdgcn_readfirstlane(ylen[r]);
    const unsigned char *q = Q + r * ALN_QBYTES;
    u32 d;
    switch ((ly + 15) >> 4) {
      case 0: d = 0u; break;                                                // nothing to align with
      case 1: d = alnl_row<1>(q, xb, tid, xnpad, lx, lxmax, gap, oe, bias); break;
      case 2: d = alnl_row<2>(q, xb, tid, xnpad, lx, lxmax, gap, oe, bias); break;
      case 3: d = alnl_row<3>(q, xb, tid, xnpad, lx, lxmax, gap, oe, bias); break;
      case 4: d = alnl_row<4>(q, xb, tid, xnpad, lx, lxmax, gap, oe, bias); break;
      case 5: d = alnl_row<5>(q, xb, tid, xnpad, lx, lxmax, gap, oe, bias); break;
      case 6: d = alnl_row<6>(q, xb, tid, xnpad, lx, lxmax, gap, oe, bias); break;
      case 7: d = alnl_row<7>(q, xb, tid, xnpad, lx, lxmax, gap, oe, bias); break;
      default: d = alnl_row<8>(q, xb, tid, xnpad, lx, lxmax, gap, oe, bias); break;
    }
    if (tid < left_cols) (out + row * ldo + ct * ALN_THREADS)[tid] = (OUT)d;
  }
}

extern "C" {

int pg_alignment_local_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                             int64_t y_npad, int yl, const int8_t *score_i8, int gap, int gap_open, void *out, int64_t ldo,
                             int out_elem_bytes, void *stream) {
  if (!x_packed || !y_packed || !score_i8 || !out || n <= 0 || m <= 0 || xl <= 0 || yl <= 0 || ldo < n)
    return pg_fail(PG_E_BADARG, "pg_alignment_local_dense: bad argument");
  if (xl > ALN_MAX_L || yl > ALN_MAX_L) return pg_fail(PG_E_TOOLONG, "pg_alignment_local_dense: at most 128 positions");
  if (gap < 1 || gap > 255) return pg_fail(PG_E_BADARG, "pg_alignment_local_dense: gap must be in 1..255");
  if (gap_open < 0 || gap_open > 255) return pg_fail(PG_E_BADARG, "pg_alignment_local_dense: gap_open must be in 0..255");
  if (x_npad < n || x_npad % 256 || y_npad < m) return pg_fail(PG_E_BADARG, "pg_alignment_local_dense: bad npad");
  if (out_elem_bytes != 2 && out_elem_bytes != 8)
    return pg_fail(PG_E_BADARG, "pg_alignment_local_dense: out_elem_bytes must be 2 (fp16) or 8");
  const long long colTiles = (n + ALN_THREADS - 1) / ALN_THREADS;
  const long long blocks = colTiles * ((m + ALN_ROWS - 1) / ALN_ROWS);
  if (blocks > 0x7fffffffll) return pg_fail(PG_E_BADARG, "pg_alignment_local_dense: too many pairs for one launch");
  const dim3 grid((unsigned)blocks), block(ALN_THREADS);
  if (out_elem_bytes == 2)
    pg_aln_local_dense_kernel<_Float16><<<grid, block, 0, (hipStream_t)stream>>>(
        (const u32 *)x_packed, n, x_npad, xl, (const u32 *)y_packed, m, y_npad, yl, (const signed char *)score_i8, (u32)gap,
        (u32)gap_open, (_Float16 *)out, ldo, colTiles);
  else
    pg_aln_local_dense_kernel<long long><<<grid, block, 0, (hipStream_t)stream>>>(
        (const u32 *)x_packed, n, x_npad, xl, (const u32 *)y_packed, m, y_npad, yl, (const signed char *)score_i8, (u32)gap,
        (u32)gap_open, (long long *)out, ldo, colTiles);
  return pg_launched("pg_alignment_local_dense");
}

}  // extern "C"
