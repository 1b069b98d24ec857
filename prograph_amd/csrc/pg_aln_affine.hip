// Gapped alignment distance with AFFINE gap penalties (global alignment, Gotoh's three-matrix recurrence): a maximal
// run of g unaligned symbols of one sequence costs gap_open + g * gap.  With e = gap, o = gap_open:
//     H[0][0] = 0,  H[0][j] = o + j e,  H[i][0] = o + i e,
//     E[i][j] = min(E[i-1][j] + e, H[i-1][j] + o + e)        run ending in a gap against x_i  (E[0][j] = inf)
//     F[i][j] = min(F[i][j-1] + e, H[i][j-1] + o + e)        run ending in a gap against y_j  (F[i][0] = inf)
//     H[i][j] = min(H[i-1][j-1] + C[x_i][y_j], E[i][j], F[i][j]),                              d(y, x) = H[lx][ly]
// BUILD DEFINED, as the linear form in pg_aln.hip, whose shape this kernel keeps: one X sequence per lane, ALN_ROWS
// wave-uniform Y rows per workgroup, their query profiles Q[r][a][j] = C[a][y_{r,j}] in LDS at stride ALN_QSTRIDE, one
// 16-byte LDS read per 16 cells, a compile-time switch on NC = ceil(ly / 16), the lengths found here, lanes past their
// own length masked out, H[ly] picked by wave-uniform selects.  The staging code below is that kernel's, repeated here
// so that pg_aln.hip stays as it is.
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
#include "pg_common.h"
#include "../../include/prograph_hip.h"

#define ALN_THREADS 256
#define ALN_ROWS 8                 // Y rows per workgroup: 8 profiles = 36 KiB of LDS
#define ALN_MAX_L 128
#define ALN_QSTRIDE 144
#define ALN_QBYTES (32 * ALN_QSTRIDE)
#define ALN_CSTRIDE 36             // bytes per row of the staged cost table (as in pg_sub.hip)

#ifndef ALN_AFFINE_LAYOUT
#define ALN_AFFINE_LAYOUT 0
#endif
#ifndef ALN_AFFINE_SPLIT
#define ALN_AFFINE_SPLIT 4
#endif

// index of the last non-zero byte + 1 over the dwords of one sequence, 0 for an empty one
__device__ __forceinline__ int alna_len_step(int len, u32 w, int g) { return w ? 4 * g + 4 - (__clz(w) >> 3) : len; }

// H and E as halves of one dword
template <int NC>
__device__ __forceinline__ u32 alna_row_packed(const unsigned char *Q, const u32 *xp, long long xnpad, int lx, int lxmax, int ly,
                                               u32 e, u32 o) {
  const u32 oe = o + e, K = oe | (e << 16);
  u32 P[16 * NC + 1];
  P[0] = 0;
#pragma unroll
  for (int j = 1; j <= 16 * NC; ++j) P[j] = (o + (u32)j * e) | ((2 * o + (u32)j * e) << 16);
  u32 xw = 0, h0 = o;
  for (int i = 0; i < lxmax; ++i) {
    if ((i & 3) == 0) xw = xp[(long long)(i >> 2) * xnpad];               // wave-uniform branch, coalesced load
    const u32 x = (xw >> (8 * (i & 3))) & 31u;
    h0 += e;                                                              // H[i + 1][0] = o + (i + 1) e
    if (i < lx) {
      const unsigned char *q = Q + x * ALN_QSTRIDE;
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
__device__ __forceinline__ u32 alna_row_wide(const unsigned char *Q, const u32 *xp, long long xnpad, int lx, int lxmax, int ly,
                                             u32 e, u32 o) {
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
  for (int i = 0; i < lxmax; ++i) {
    if ((i & 3) == 0) xw = xp[(long long)(i >> 2) * xnpad];               // wave-uniform branch, coalesced load
    const u32 x = (xw >> (8 * (i & 3))) & 31u;
    h0 += e;
    if (i < lx) {
      const unsigned char *q = Q + x * ALN_QSTRIDE;
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
__device__ __forceinline__ u32 alna_row(const unsigned char *Q, const u32 *xp, long long xnpad, int lx, int lxmax, int ly, u32 e,
                                        u32 o) {
  if (ALN_AFFINE_LAYOUT == 1 || (ALN_AFFINE_LAYOUT == 2 && NC <= ALN_AFFINE_SPLIT))
    return alna_row_wide<NC>(Q, xp, xnpad, lx, lxmax, ly, e, o);
  return alna_row_packed<NC>(Q, xp, xnpad, lx, lxmax, ly, e, o);
}

template <typename OUT>
__global__ __launch_bounds__(ALN_THREADS) void pg_aln_affine_dense_kernel(const u32 *__restrict__ xt, long long n, long long xnpad,
                                                                          int xl, const u32 *__restrict__ yt, long long m,
                                                                          long long ynpad, int yl,
                                                                          const unsigned char *__restrict__ cost, u32 gap, u32 open,
                                                                          OUT *__restrict__ out, long long ldo, long long colTiles) {
  __shared__ __attribute__((aligned(16))) unsigned char Q[ALN_ROWS * ALN_QBYTES];
  __shared__ u32 ytile[ALN_ROWS][ALN_MAX_L / 4];
  __shared__ unsigned char cs[32 * ALN_CSTRIDE];
  __shared__ int ylen[ALN_ROWS];
  const int tid = threadIdx.x;
  const long long ct = (long long)blockIdx.x % colTiles, rg = (long long)blockIdx.x / colTiles;
  const long long row0 = rg * ALN_ROWS;
  const int xg = (xl + 3) >> 2, yg = (yl + 3) >> 2;                         // <= 32 dwords each (the host checks)

  for (int i = tid; i < 1024; i += ALN_THREADS) cs[(i >> 5) * ALN_CSTRIDE + (i & 31)] = cost[i];
  for (int i = tid; i < ALN_ROWS * (ALN_MAX_L / 4); i += ALN_THREADS) {
    const int r = i >> 5, g = i & 31;
    ytile[r][g] = (row0 + r < m && g < yg) ? yt[(long long)g * ynpad + row0 + r] : 0u;
  }
  __syncthreads();
  if (tid < ALN_ROWS) {
    int len = 0;
    for (int g = 0; g < ALN_MAX_L / 4; ++g) len = alna_len_step(len, ytile[tid][g], g);
    ylen[tid] = len;
  }
  for (int i = tid; i < ALN_ROWS * 32 * 32; i += ALN_THREADS) {
    const int g = i & 31, a = (i >> 5) & 31, r = i >> 10;
    const u32 w = ytile[r][g];
    const unsigned char *crow = cs + a * ALN_CSTRIDE;                       // C is symmetric: C[a][y] = C[y][a]
    const u32 d = (u32)crow[w & 31u] | ((u32)crow[(w >> 8) & 31u] << 8) | ((u32)crow[(w >> 16) & 31u] << 16) |
                  ((u32)crow[(w >> 24) & 31u] << 24);
    *(u32 *)(Q + r * ALN_QBYTES + a * ALN_QSTRIDE + 4 * g) = d;
  }
  __syncthreads();

  const long long col = ct * ALN_THREADS + tid;                             // < colTiles * 256 <= xnpad
  const bool have = col < n;
  const u32 *xp = xt + col;
  int lx = 0;
  for (int g = 0; g < xg; ++g) lx = alna_len_step(lx, xp[(long long)g * xnpad], g);
  if (!have) lx = 0;
  int lxmax = lx;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) lxmax = max(lxmax, __shfl_xor(lxmax, s));
  lxmax = __builtin_amdgcn_readfirstlane(lxmax);

  for (int r = 0; r < ALN_ROWS; ++r) {
    const long long row = row0 + r;
    if (row >= m) break;
    const int ly = __builtin_amdgcn_readfirstlane(ylen[r]);
    const unsigned char *q = Q + r * ALN_QBYTES;
    u32 d;
    switch ((ly + 15) >> 4) {
      case 0: d = lx ? open + (u32)lx * gap : 0u; break;                    // one run of lx symbols, or nothing
      case 1: d = alna_row<1>(q, xp, xnpad, lx, lxmax, ly, gap, open); break;
      case 2: d = alna_row<2>(q, xp, xnpad, lx, lxmax, ly, gap, open); break;
      case 3: d = alna_row<3>(q, xp, xnpad, lx, lxmax, ly, gap, open); break;
      case 4: d = alna_row<4>(q, xp, xnpad, lx, lxmax, ly, gap, open); break;
      case 5: d = alna_row<5>(q, xp, xnpad, lx, lxmax, ly, gap, open); break;
      case 6: d = alna_row<6>(q, xp, xnpad, lx, lxmax, ly, gap, open); break;
      case 7: d = alna_row<7>(q, xp, xnpad, lx, lxmax, ly, gap, open); break;
      default: d = alna_row<8>(q, xp, xnpad, lx, lxmax, ly, gap, open); break;
    }
    if (have) out[row * ldo + col] = (OUT)d;
  }
}

extern "C" {

int pg_alignment_affine_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                              int64_t y_npad, int yl, const uint8_t *cost_u8, int gap, int gap_open, void *out, int64_t ldo,
                              int out_elem_bytes, void *stream) {
  if (!x_packed || !y_packed || !cost_u8 || !out || n <= 0 || m <= 0 || xl <= 0 || yl <= 0 || ldo < n)
    return pg_fail(PG_E_BADARG, "pg_alignment_affine_dense: bad argument");
  if (xl > ALN_MAX_L || yl > ALN_MAX_L) return pg_fail(PG_E_TOOLONG, "pg_alignment_affine_dense: at most 128 positions");
  if (gap < 1 || gap > 255) return pg_fail(PG_E_BADARG, "pg_alignment_affine_dense: gap must be in 1..255");
  if (gap_open < 0 || gap_open > 255) return pg_fail(PG_E_BADARG, "pg_alignment_affine_dense: gap_open must be in 0..255");
  if (x_npad < n || x_npad % 256 || y_npad < m) return pg_fail(PG_E_BADARG, "pg_alignment_affine_dense: bad npad");
  if (out_elem_bytes != 2 && out_elem_bytes != 8)
    return pg_fail(PG_E_BADARG, "pg_alignment_affine_dense: out_elem_bytes must be 2 (fp16) or 8");
  const long long colTiles = (n + ALN_THREADS - 1) / ALN_THREADS;
  const long long blocks = colTiles * ((m + ALN_ROWS - 1) / ALN_ROWS);
  if (blocks > 0x7fffffffll) return pg_fail(PG_E_BADARG, "pg_alignment_affine_dense: too many pairs for one launch");
  const dim3 grid((unsigned)blocks), block(ALN_THREADS);
  if (out_elem_bytes == 2)
    pg_aln_affine_dense_kernel<_Float16><<<grid, block, 0, (hipStream_t)stream>>>(
        (const u32 *)x_packed, n, x_npad, xl, (const u32 *)y_packed, m, y_npad, yl, cost_u8, (u32)gap, (u32)gap_open, (_Float16 *)out,
        ldo, colTiles);
  else
    pg_aln_affine_dense_kernel<long long><<<grid, block, 0, (hipStream_t)stream>>>(
        (const u32 *)x_packed, n, x_npad, xl, (const u32 *)y_packed, m, y_npad, yl, cost_u8, (u32)gap, (u32)gap_open, (long long *)out,
        ldo, colTiles);
  return pg_launched("pg_alignment_affine_dense");
}

}  // extern "C"
