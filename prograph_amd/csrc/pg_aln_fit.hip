// FIT ("glocal") alignment score with Gotoh's affine gaps: ALL of y is aligned, within ANY substring of x - only the ends of
// x are free.  Under a symmetric SCORE table S (larger is nearer), e = gap, o = gap_open, i over x and j over y:
//     H[i][0] = 0,  H[0][j] = -(o + j e) (j >= 1),  E[0][j] = F[i][0] = -inf,
//     E[i][j] = max(E[i-1][j] - e, H[i-1][j] - o - e),   F[i][j] = max(F[i][j-1] - e, H[i][j-1] - o - e),
//     H[i][j] = max(H[i-1][j-1] + S[x_i][y_j], E[i][j], F[i][j])                                     (no zero floor),
//     s(y, x) = max over i = 0..len x of H[i][len y].
// BUILD DEFINED.  A similarity, NOT symmetric, and it may be negative: -(o + e len y) <= s <= min(len x, len y) max S.
// Two kernels in the shape of pg_aln_semiglobal.hip: pg_aln_fit_dense_kernel up to 128 positions (one X sequence per lane,
// ALN_ROWS wave-uniform Y rows per workgroup, byte query profiles in LDS at stride ALN_QSTRIDE, one 16-byte LDS read per 16
// cells, P[j] = H | E << 16, a compile-time switch on NC = ceil(ly / 16), the lengths found here, lanes past their own
// length masked out) and pg_aln_fit_long_dense_kernel, the strips, boundary column and profile slots of pg_aln_long.hip up
// to 2048.  The staging code is those kernels', repeated here so that they stay as they are.
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
#include "pg_common.h"
#include "../../include/prograph_hip.h"

#define ALN_THREADS 256
#define ALN_ROWS 8                 // Y rows per workgroup: 8 profiles = 36 KiB of LDS (long kernel: 8 strips of one row)
#define ALN_MAX_L 128
#define ALN_STRIP 128
#define ALN_QSTRIDE 144
#define ALN_QBYTES (32 * ALN_QSTRIDE)
#define ALN_CSTRIDE 36             // bytes per row of the staged score table (as in pg_sub.hip)
#define ALNG_MAX_L PG_ALN_LONG_MAX_L

typedef unsigned short alnf_u16x2 __attribute__((ext_vector_type(2)));

// index of the last non-zero byte + 1 of dword g, 0 for an empty dword
__device__ __forceinline__ int alnf_len(u32 w, int g) { return w ? 4 * g + 4 - (__clz(w) >> 3) : 0; }

// a - b, 0 where b > a
__device__ __forceinline__ u32 alnf_sat(u32 a, u32 b) { return __builtin_elementwise_sub_sat(a, b); }

// the same on both 16-bit halves at once
__device__ __forceinline__ u32 alnf_sat2(u32 a, u32 b) {
  return __builtin_bit_cast(u32, __builtin_elementwise_sub_sat(__builtin_bit_cast(alnf_u16x2, a), __builtin_bit_cast(alnf_u16x2, b)));
}

// H[0][j] + Z: Z at j = 0, Z - (o + j e) beyond (0 past the operand's width, where it is padding)
__device__ __forceinline__ u32 alnf_row0(u32 Z, u32 o, u32 e, int j) { return j ? alnf_sat(Z, o + (u32)j * e) : Z; }

// One strip of 16 * NC cells of one Y row against the lane's X sequence: the whole row in the short kernel (j0 = 0, LAST),
// strip j0 / 128 in the long one.  Q: the strip's profile; jl: the index of len y inside the LAST strip's last chunk
// (1..16); wsb: the boundary column (read when j0 > 0, written unless LAST); best: the maximum so far (+ Z).
template <int NC, bool LAST, bool LONG>
__device__ __forceinline__ u32 alnf_strip(const unsigned char *Q, const u32 *xb, u32 *wsb, int lane, long long xnpad, int lx, int lxmax,
                                          int j0, int jl, u32 e, u32 oe, u32 bias, u32 Z, u32 best) {
  const u32 K = oe | (e << 16);
  u32 m[16];                                                              // scalar masks: all ones at len y
#pragma unroll
  for (int t = 0; t < 16; ++t) m[t] = (LAST && jl == t + 1) ? 0xffffffffu : 0u;
  u32 P[16 * NC + 1];                                                     // P[j] = H[j0 + j] | E[j0 + j] << 16, + Z each; P[0]: H alone
  P[0] = alnf_row0(Z, oe - e, e, j0);                                     // row 0: H = -(o + j e), E = -inf
  P[1] = alnf_row0(Z, oe - e, e, j0 + 1);
#pragma unroll
  for (int j = 2; j <= 16 * NC; ++j) P[j] = alnf_sat(P[j - 1], e);        // a chain: one subtraction a column, 0 stays 0
  u32 xw = 0;
  for (int i = 0; i < lxmax; ++i) {
    if ((i & 3) == 0) xw = (xb + (long long)(i >> 2) * xnpad)[lane];          // wave-uniform branch and base, coalesced load
    const u32 x = (xw >> (8 * (i & 3))) & 31u;
    if (i < lx) {
      const unsigned char *q = Q + x * ALN_QSTRIDE;
      u32 left = Z, F = 0;                                                // H[i][0] = 0, F[i][0] = -inf
      u32 *bd = LONG ? wsb + (long long)i * ALN_THREADS : nullptr;        // this step's line of the boundary column
      if (LONG && j0) {                                                   // wave-uniform
        const u32 v = bd[lane];
        left = v & 0xffffu;
        F = v >> 16;
      }
      u32 diag = P[0];
      P[0] = left;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const uint4 v = *(const uint4 *)(q + 16 * c);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
        // the diagonal terms first, from the old column: afterwards every cell is rewritten in place
        u32 T[16];
        T[0] = alnf_sat((diag & 0xffffu) + (w[0] & 255u), bias);
#pragma unroll
        for (int t = 1; t < 16; ++t) T[t] = alnf_sat((P[16 * c + t] & 0xffffu) + ((w[t >> 2] >> (8 * (t & 3))) & 255u), bias);
        diag = P[16 * c + 16];
#pragma unroll
        for (int t = 0; t < 16; t += 2) {
          u32 h[2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const u32 s = alnf_sat2(P[16 * c + t + u + 1], K);            // H -sat- (o + e) | (E -sat- e) << 16
            const u32 E = max(s & 0xffffu, s >> 16);
            F = max(alnf_sat(F, e), alnf_sat(left, oe));
            left = max(T[t + u], max(E, F));
            P[16 * c + t + u + 1] = left | (E << 16);
            h[u] = left;
          }
          if (LAST && c == NC - 1) best = max(max(best, h[0] & m[t]), h[1] & m[t + 1]);      // H[i][len y] alone
        }
      }
      if (LONG && !LAST) bd[lane] = left | (F << 16);                     // H[i + 1][j0 + 128] | F[i + 1][j0 + 128] << 16
    }
  }
  return best;                                                            // row len x is NOT folded: all of y must align
}

// the score table into LDS as bytes S + bias; returns bias = -min(0, min S) and *top = max(0, max S), both wave-uniform
__device__ __forceinline__ u32 alnf_table(const signed char *score, unsigned char *cs, int *smin, int *smax, int tid, u32 *top) {
  if (tid == 0) {
    *smin = 0;
    *smax = 0;
  }
  int sc[4], lo = 0, hi = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    sc[k] = score[tid + k * ALN_THREADS];
    lo = min(lo, sc[k]);
    hi = max(hi, sc[k]);
  }
  __syncthreads();
  if (lo < 0) atomicMin(smin, lo);
  if (hi > 0) atomicMax(smax, hi);
  __syncthreads();
  const u32 bias = (u32)(-__builtin_amdgcn_readfirstlane(*smin));            // 0..128, in a scalar register
  *top = (u32)__builtin_amdgcn_readfirstlane(*smax);                        // 0..127
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = tid + k * ALN_THREADS;
    cs[(i >> 5) * ALN_CSTRIDE + (i & 31)] = (unsigned char)(sc[k] + (int)bias);
  }
  return bias;
}

// four profile bytes of symbol row `crow` against the tokens of dword w, positions past the sequence (keep < 4) zeroed
__device__ __forceinline__ u32 alnf_profile(const unsigned char *crow, u32 w, int keep) {
  const u32 d = (u32)crow[w & 31u] | ((u32)crow[(w >> 8) & 31u] << 8) | ((u32)crow[(w >> 16) & 31u] << 16) |
                ((u32)crow[(w >> 24) & 31u] << 24);
  return d & (keep >= 4 ? 0xffffffffu : keep <= 0 ? 0u : (1u << (8 * keep)) - 1u);
}

template <typename OUT>
__global__ __launch_bounds__(ALN_THREADS) __attribute__((amdgpu_waves_per_eu(3))) void pg_aln_fit_dense_kernel(
    const u32 *__restrict__ xt, long long n, long long xnpad, int xl, const u32 *__restrict__ yt, long long m, long long ynpad,
    int yl, const signed char *__restrict__ score, u32 gap, u32 open, int obias, OUT *__restrict__ out, long long ldo,
    long long colTiles) {
  __shared__ __attribute__((aligned(16))) unsigned char Q[ALN_ROWS * ALN_QBYTES];
  __shared__ u32 ytile[ALN_ROWS][ALN_MAX_L / 4];
  __shared__ unsigned char cs[32 * ALN_CSTRIDE];
  __shared__ int ylen[ALN_ROWS];
  __shared__ int smin, smax;
  const int tid = threadIdx.x;
  const long long ct = (long long)blockIdx.x % colTiles, rg = (long long)blockIdx.x / colTiles;
  const long long row0 = rg * ALN_ROWS;
  const int xg = (xl + 3) >> 2, yg = (yl + 3) >> 2;                         // <= 32 dwords each (the host checks)

  for (int i = tid; i < ALN_ROWS * (ALN_MAX_L / 4); i += ALN_THREADS) {
    const int r = i >> 5, g = i & 31;
    ytile[r][g] = (row0 + r < m && g < yg) ? yt[(long long)g * ynpad + row0 + r] : 0u;
  }
  u32 top;
  const u32 bias = alnf_table(score, cs, &smin, &smax, tid, &top);          // its barriers cover ytile
  if (tid < ALN_ROWS) {
    int len = 0;
    for (int g = 0; g < ALN_MAX_L / 4; ++g) len = max(len, alnf_len(ytile[tid][g], g));
    ylen[tid] = len;
  }
  __syncthreads();
  for (int i = tid; i < ALN_ROWS * 32 * 32; i += ALN_THREADS) {
    const int g = i & 31, a = (i >> 5) & 31, r = i >> 10;
    // S is symmetric: S[a][y] = S[y][a]; past len y: byte 0, a score of -bias
    *(u32 *)(Q + r * ALN_QBYTES + a * ALN_QSTRIDE + 4 * g) = alnf_profile(cs + a * ALN_CSTRIDE, ytile[r][g], ylen[r] - 4 * g);
  }
  __syncthreads();

  // column ct * 256 + tid (< colTiles * 256 <= xnpad): a wave-uniform base and the lane, so that one VGPR addresses both
  // the tokens and the output
  const u32 *xb = xt + ct * ALN_THREADS;
  const long long left_cols = n - ct * ALN_THREADS;                         // >= 1
  int lx = 0;
  for (int g = 0; g < xg; ++g) lx = max(lx, alnf_len((xb + (long long)g * xnpad)[tid], g));
  if (tid >= left_cols) lx = 0;
  int lxmax = lx;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) lxmax = max(lxmax, __shfl_xor(lxmax, s));
  lxmax = __builtin_amdgcn_readfirstlane(lxmax);

  const u32 oe = open + gap, Z = open + (u32)yl * (gap + top);              // o + yl (e + 2 top) + 255 <= 65 535: the caller's guarantee
  for (int r = 0; r < ALN_ROWS; ++r) {
    const long long row = row0 + r;
    if (row >= m) break;
    const int ly = __builtin_amdgcn_readfirstlane(ylen[r]);
    const unsigned char *q = Q + r * ALN_QBYTES;
    const int jl = ly - ((ly - 1) & ~15);                                   // 1..16 for ly >= 1
    // Row 0 differs from column to column but not from row to row of Y: left to itself the compiler forms all 129 values
    // once, ahead of this loop, and keeps them alive across it - beyond the 168 registers of three waves per SIMD.  The
    // empty statement makes this row's Z a value of its own, so row 0 is formed where it is used.
    u32 zr = Z;
    asm volatile("" : "+s"(zr));
    const u32 first = alnf_row0(zr, open, gap, ly);                         // H[0][len y]
    u32 d;
#define ALNF_ROW(NC) alnf_strip<NC, true, false>(q, xb, nullptr, tid, xnpad, lx, lxmax, 0, jl, gap, oe, bias, zr, first)
    switch ((ly + 15) >> 4) {
      case 0: d = Z; break;                                                 // nothing to align: 0
      case 1: d = ALNF_ROW(1); break;
      case 2: d = ALNF_ROW(2); break;
      case 3: d = ALNF_ROW(3); break;
      case 4: d = ALNF_ROW(4); break;
      case 5: d = ALNF_ROW(5); break;
      case 6: d = ALNF_ROW(6); break;
      case 7: d = ALNF_ROW(7); break;
      default: d = ALNF_ROW(8); break;
    }
#undef ALNF_ROW
    if (tid < left_cols) (out + row * ldo + ct * ALN_THREADS)[tid] = (OUT)((int)d - (int)Z + obias);
  }
}

// Beyond 128 positions: pg_aln_long.hip's loop over (column tile, row group) items, one Y row at a time, its strips in
// groups of eight profile slots, the boundary column of workgroup b in slice b of the workspace.
template <typename OUT>
__global__ __launch_bounds__(ALN_THREADS) void pg_aln_fit_long_dense_kernel(
    const u32 *__restrict__ xt, long long n, long long xnpad, int xl, const u32 *__restrict__ yt, long long m, long long ynpad,
    int yl, const signed char *__restrict__ score, u32 gap, u32 open, int obias, OUT *__restrict__ out, long long ldo,
    int colTiles, int items, u32 *ws) {
  __shared__ __attribute__((aligned(16))) unsigned char Q[ALN_ROWS * ALN_QBYTES];
  __shared__ u32 yrow[ALNG_MAX_L / 4];
  __shared__ unsigned char cs[32 * ALN_CSTRIDE];
  __shared__ int ylen;
  __shared__ int smin, smax;
  const int tid = threadIdx.x;
  const int xg = (xl + 3) >> 2, yg = (yl + 3) >> 2;                         // <= 512 dwords each (the host checks)
  u32 top;
  const u32 bias = alnf_table(score, cs, &smin, &smax, tid, &top);
  const u32 oe = open + gap, Z = open + (u32)yl * (gap + top);              // o + yl (e + 2 top) + 255 <= 65 535: the caller's guarantee

  u32 *wsb = ws + (long long)blockIdx.x * (xg * 4 * ALN_THREADS);          // this workgroup's boundary column
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const long long ct = item % colTiles, row0 = (long long)(item / colTiles) * ALN_ROWS;
    const u32 *xb = xt + ct * ALN_THREADS;
    const long long left_cols = n - ct * ALN_THREADS;                       // >= 1
    int lx = 0;
    for (int g = 0; g < xg; ++g) lx = max(lx, alnf_len((xb + (long long)g * xnpad)[tid], g));
    if (tid >= left_cols) lx = 0;
    int lxmax = lx;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) lxmax = max(lxmax, __shfl_xor(lxmax, s));
    lxmax = __builtin_amdgcn_readfirstlane(lxmax);

    for (int r = 0; r < ALN_ROWS; ++r) {
      const long long row = row0 + r;
      if (row >= m) break;
      __syncthreads();                                                    // the previous row's readers of Q / yrow / ylen are done
      if (tid == 0) ylen = 0;
      __syncthreads();
      for (int g = tid; g < ALNG_MAX_L / 4; g += ALN_THREADS) {
        const u32 w = g < yg ? yt[(long long)g * ynpad + row] : 0u;
        yrow[g] = w;
        if (w) atomicMax(&ylen, alnf_len(w, g));
      }
      __syncthreads();
      const int ly = __builtin_amdgcn_readfirstlane(ylen);
      const int ns = (ly + ALN_STRIP - 1) / ALN_STRIP;                    // strips that hold a position of the row
      u32 best = alnf_row0(Z, open, gap, ly);                             // H[0][len y]; carried from strip to strip
      for (int s0 = 0; s0 < ns; s0 += ALN_ROWS) {
        const int nb = min(ALN_ROWS, ns - s0);
        if (s0) __syncthreads();                                          // the previous eight strips' profiles are read
        for (int i = tid; i < nb * 32 * 32; i += ALN_THREADS) {
          const int g = i & 31, a = (i >> 5) & 31, slot = i >> 10;
          const int gy = (s0 + slot) * (ALN_STRIP / 4) + g;               // < 512
          *(u32 *)(Q + slot * ALN_QBYTES + a * ALN_QSTRIDE + 4 * g) = alnf_profile(cs + a * ALN_CSTRIDE, yrow[gy], ly - 4 * gy);
        }
        __syncthreads();
        for (int s = s0; s < s0 + nb; ++s) {
          const unsigned char *q = Q + (s - s0) * ALN_QBYTES;
          const int j0 = s * ALN_STRIP;
          if (s < ns - 1) {
            best = alnf_strip<8, false, true>(q, xb, wsb, tid, xnpad, lx, lxmax, j0, 0, gap, oe, bias, Z, best);
            continue;
          }
          const int rest = ly - j0, jl = rest - ((rest - 1) & ~15);       // 1..128, 1..16
#define ALNF_LAST(NC) alnf_strip<NC, true, true>(q, xb, wsb, tid, xnpad, lx, lxmax, j0, jl, gap, oe, bias, Z, best)
          switch ((rest + 15) >> 4) {
            case 1: best = ALNF_LAST(1); break;
            case 2: best = ALNF_LAST(2); break;
            case 3: best = ALNF_LAST(3); break;
            case 4: best = ALNF_LAST(4); break;
            case 5: best = ALNF_LAST(5); break;
            case 6: best = ALNF_LAST(6); break;
            case 7: best = ALNF_LAST(7); break;
            default: best = ALNF_LAST(8); break;
          }
#undef ALNF_LAST
        }
      }
      if (tid < left_cols) (out + row * ldo + ct * ALN_THREADS)[tid] = (OUT)((int)best - (int)Z + obias);
    }
  }
}

// the two entries' 16-bit cells: o + yl (e + 2 top) + 255, top from the table on the device - the caller tests it on the host
extern "C" {

int pg_alignment_fit_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                           int64_t y_npad, int yl, const int8_t *score_i8, int gap, int gap_open, int bias, void *out,
                           int64_t ldo, int out_elem_bytes, void *stream) {
  if (!x_packed || !y_packed || !score_i8 || !out || n <= 0 || m <= 0 || xl <= 0 || yl <= 0 || ldo < n)
    return pg_fail(PG_E_BADARG, "pg_alignment_fit_dense: bad argument");
  if (xl > ALN_MAX_L || yl > ALN_MAX_L) return pg_fail(PG_E_TOOLONG, "pg_alignment_fit_dense: at most 128 positions");
  if (gap < 1 || gap > 255) return pg_fail(PG_E_BADARG, "pg_alignment_fit_dense: gap must be in 1..255");
  if (gap_open < 0 || gap_open > 255) return pg_fail(PG_E_BADARG, "pg_alignment_fit_dense: gap_open must be in 0..255");
  if (bias < 0) return pg_fail(PG_E_BADARG, "pg_alignment_fit_dense: bias must not be negative");
  if (x_npad < n || x_npad % 256 || y_npad < m) return pg_fail(PG_E_BADARG, "pg_alignment_fit_dense: bad npad");
  if (out_elem_bytes != 2 && out_elem_bytes != 8)
    return pg_fail(PG_E_BADARG, "pg_alignment_fit_dense: out_elem_bytes must be 2 (fp16) or 8");
  const long long colTiles = (n + ALN_THREADS - 1) / ALN_THREADS;
  const long long blocks = colTiles * ((m + ALN_ROWS - 1) / ALN_ROWS);
  if (blocks > 0x7fffffffll) return pg_fail(PG_E_BADARG, "pg_alignment_fit_dense: too many pairs for one launch");
  const dim3 grid((unsigned)blocks), block(ALN_THREADS);
  if (out_elem_bytes == 2)
    pg_aln_fit_dense_kernel<_Float16><<<grid, block, 0, (hipStream_t)stream>>>(
        (const u32 *)x_packed, n, x_npad, xl, (const u32 *)y_packed, m, y_npad, yl, (const signed char *)score_i8, (u32)gap,
        (u32)gap_open, bias, (_Float16 *)out, ldo, colTiles);
  else
    pg_aln_fit_dense_kernel<long long><<<grid, block, 0, (hipStream_t)stream>>>(
        (const u32 *)x_packed, n, x_npad, xl, (const u32 *)y_packed, m, y_npad, yl, (const signed char *)score_i8, (u32)gap,
        (u32)gap_open, bias, (long long *)out, ldo, colTiles);
  return pg_launched("pg_alignment_fit_dense");
}

int pg_alignment_fit_long_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                                int64_t y_npad, int yl, const int8_t *score_i8, int gap, int gap_open, int bias, void *out,
                                int64_t ldo, int out_elem_bytes, void *workspace, int64_t workspace_bytes, void *stream) {
  if (!x_packed || !y_packed || !score_i8 || !out || !workspace || n <= 0 || m <= 0 || xl <= 0 || yl <= 0 || ldo < n)
    return pg_fail(PG_E_BADARG, "pg_alignment_fit_long_dense: bad argument");
  if (xl > ALNG_MAX_L || yl > ALNG_MAX_L) return pg_fail(PG_E_TOOLONG, "pg_alignment_fit_long_dense: at most 2048 positions");
  if (gap < 1 || gap > 255) return pg_fail(PG_E_BADARG, "pg_alignment_fit_long_dense: gap must be in 1..255");
  if (gap_open < 0 || gap_open > 255) return pg_fail(PG_E_BADARG, "pg_alignment_fit_long_dense: gap_open must be in 0..255");
  if (bias < 0) return pg_fail(PG_E_BADARG, "pg_alignment_fit_long_dense: bias must not be negative");
  if (x_npad < n || x_npad % 256 || y_npad < m) return pg_fail(PG_E_BADARG, "pg_alignment_fit_long_dense: bad npad");
  if (out_elem_bytes != 4 && out_elem_bytes != 8)
    return pg_fail(PG_E_BADARG, "pg_alignment_fit_long_dense: out_elem_bytes must be 4 (int32) or 8");
  const long long one = (long long)ALN_THREADS * (((xl + 3) / 4) * 4) * 4;  // pg_alignment_long_workspace's share
  if (workspace_bytes < one)
    return pg_fail(PG_E_BADARG, "pg_alignment_fit_long_dense: the workspace is smaller than one workgroup's share");
  const long long colTiles = (n + ALN_THREADS - 1) / ALN_THREADS;
  const long long items = colTiles * ((m + ALN_ROWS - 1) / ALN_ROWS);
  long long blocks = workspace_bytes / one;                                 // as many workgroups as the workspace holds
  if (items > 0x7fffffffll) return pg_fail(PG_E_BADARG, "pg_alignment_fit_long_dense: too many pairs for one launch");
  if (blocks > items) blocks = items;
  const dim3 grid((unsigned)blocks), block(ALN_THREADS);
  if (out_elem_bytes == 4)
    pg_aln_fit_long_dense_kernel<int><<<grid, block, 0, (hipStream_t)stream>>>(
        (const u32 *)x_packed, n, x_npad, xl, (const u32 *)y_packed, m, y_npad, yl, (const signed char *)score_i8, (u32)gap,
        (u32)gap_open, bias, (int *)out, ldo, (int)colTiles, (int)items, (u32 *)workspace);
  else
    pg_aln_fit_long_dense_kernel<long long><<<grid, block, 0, (hipStream_t)stream>>>(
        (const u32 *)x_packed, n, x_npad, xl, (const u32 *)y_packed, m, y_npad, yl, (const signed char *)score_i8, (u32)gap,
        (u32)gap_open, bias, (long long *)out, ldo, (int)colTiles, (int)items, (u32 *)workspace);
  return pg_launched("pg_alignment_fit_long_dense");
}

}  // extern "C"
