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
// of a wave load 64 consecutive columns coalesced.  The lengths are found here, from the packed dwords: X once per
// lane and workgroup, Y while the profile is built - no separate length pass, no host sync.
#include "pg_common.h"
#include "../../include/prograph_hip.h"

#define ALN_THREADS 256
#define ALN_ROWS 8                 // Y rows per workgroup: 8 profiles = 36 KiB of LDS
#define ALN_MAX_L 128
#define ALN_QSTRIDE 144
#define ALN_QBYTES (32 * ALN_QSTRIDE)
#define ALN_CSTRIDE 36             // bytes per row of the staged cost table (as in pg_sub.hip)

// index of the last non-zero byte + 1 over the dwords of one sequence, 0 for an empty one
__device__ __forceinline__ int aln_len_step(int len, u32 w, int g) { return w ? 4 * g + 4 - (__clz(w) >> 3) : len; }

template <int NC>
__device__ __forceinline__ u32 aln_row(const unsigned char *Q, const u32 *xp, long long xnpad, int lx, int lxmax, int ly,
                                       u32 gap) {
  u32 H[16 * NC + 1];
#pragma unroll
  for (int j = 0; j <= 16 * NC; ++j) H[j] = (u32)j * gap;
  u32 xw = 0;
  for (int i = 0; i < lxmax; ++i) {
    if ((i & 3) == 0) xw = xp[(long long)(i >> 2) * xnpad];               // wave-uniform branch, coalesced load
    const u32 x = (xw >> (8 * (i & 3))) & 31u;
    if (i < lx) {
      const unsigned char *q = Q + x * ALN_QSTRIDE;
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

template <typename OUT>
__global__ __launch_bounds__(ALN_THREADS) void pg_aln_dense_kernel(const u32 *__restrict__ xt, long long n, long long xnpad, int xl,
                                                                   const u32 *__restrict__ yt, long long m, long long ynpad, int yl,
                                                                   const unsigned char *__restrict__ cost, u32 gap,
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
    for (int g = 0; g < ALN_MAX_L / 4; ++g) len = aln_len_step(len, ytile[tid][g], g);
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
  for (int g = 0; g < xg; ++g) lx = aln_len_step(lx, xp[(long long)g * xnpad], g);
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
      case 0: d = (u32)lx * gap; break;
      case 1: d = aln_row<1>(q, xp, xnpad, lx, lxmax, ly, gap); break;
      case 2: d = aln_row<2>(q, xp, xnpad, lx, lxmax, ly, gap); break;
      case 3: d = aln_row<3>(q, xp, xnpad, lx, lxmax, ly, gap); break;
      case 4: d = aln_row<4>(q, xp, xnpad, lx, lxmax, ly, gap); break;
      case 5: d = aln_row<5>(q, xp, xnpad, lx, lxmax, ly, gap); break;
      case 6: d = aln_row<6>(q, xp, xnpad, lx, lxmax, ly, gap); break;
      case 7: d = aln_row<7>(q, xp, xnpad, lx, lxmax, ly, gap); break;
      default: d = aln_row<8>(q, xp, xnpad, lx, lxmax, ly, gap); break;
    }
    if (have) out[row * ldo + col] = (OUT)d;
  }
}

extern "C" {

int pg_alignment_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m, int64_t y_npad,
                       int yl, const uint8_t *cost_u8, int gap, void *out, int64_t ldo, int out_elem_bytes, void *stream) {
  if (!x_packed || !y_packed || !cost_u8 || !out || n <= 0 || m <= 0 || xl <= 0 || yl <= 0 || ldo < n)
    return pg_fail(PG_E_BADARG, "pg_alignment_dense: bad argument");
  if (xl > ALN_MAX_L || yl > ALN_MAX_L) return pg_fail(PG_E_TOOLONG, "pg_alignment_dense: at most 128 positions");
  if (gap < 1 || gap > 255) return pg_fail(PG_E_BADARG, "pg_alignment_dense: gap must be in 1..255");
  if (x_npad < n || x_npad % 256 || y_npad < m) return pg_fail(PG_E_BADARG, "pg_alignment_dense: bad npad");
  if (out_elem_bytes != 2 && out_elem_bytes != 8)
    return pg_fail(PG_E_BADARG, "pg_alignment_dense: out_elem_bytes must be 2 (fp16) or 8");
  const long long colTiles = (n + ALN_THREADS - 1) / ALN_THREADS;
  const long long blocks = colTiles * ((m + ALN_ROWS - 1) / ALN_ROWS);
  if (blocks > 0x7fffffffll) return pg_fail(PG_E_BADARG, "pg_alignment_dense: too many pairs for one launch");
  const dim3 grid((unsigned)blocks), block(ALN_THREADS);
  if (out_elem_bytes == 2)
    pg_aln_dense_kernel<_Float16><<<grid, block, 0, (hipStream_t)stream>>>((const u32 *)x_packed, n, x_npad, xl, (const u32 *)y_packed, m,
                                                                          y_npad, yl, cost_u8, (u32)gap, (_Float16 *)out, ldo, colTiles);
  else
    pg_aln_dense_kernel<long long><<<grid, block, 0, (hipStream_t)stream>>>((const u32 *)x_packed, n, x_npad, xl, (const u32 *)y_packed, m,
                                                                           y_npad, yl, cost_u8, (u32)gap, (long long *)out, ldo, colTiles);
  return pg_launched("pg_alignment_dense");
}

}  // extern "C"
