// Alignment distances and local alignment scores of sequences BEYOND 128 positions (up to PG_ALN_LONG_MAX_L = 2048):
// the recurrences of pg_aln_affine.hip (global, Gotoh) and pg_aln_local.hip (Smith-Waterman, Gotoh), strip-mined along
// the Y side.  BUILD DEFINED.  One kernel template <LOCAL, OUT>, always in Gotoh form: gap_open = 0 is the linear gap
// penalty exactly (E = min(E + e, H + e)).  The shape of the 128-position kernels: one X sequence per lane, wave-uniform
// Y rows, byte query profiles in LDS at stride ALN_QSTRIDE, one 16-byte LDS read per 16 cells, H | E << 16 in one
// register per cell, the lengths found here, lanes past their own len x masked out.  The staging code is those kernels',
// repeated here so that they stay as they are.
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
#include "pg_common.h"
#include "../../include/prograph_hip.h"

#define ALN_THREADS 256
#define ALN_ROWS 8                 // Y rows per item; also the profile slots in LDS (8 strips of one row): 36 KiB
#define ALN_STRIP 128
#define ALN_QSTRIDE 144
#define ALN_QBYTES (32 * ALN_QSTRIDE)
#define ALN_CSTRIDE 36             // bytes per row of the staged table (as in pg_sub.hip)
#define ALNG_MAX_L PG_ALN_LONG_MAX_L
#define ALNG_RESIDENT 2            // workgroups per CU: the kernel takes 196..198 VGPRs, 2 waves per SIMD (profiles/aln_long_dense.txt)

typedef unsigned short alng_u16x2 __attribute__((ext_vector_type(2)));

// index of the last non-zero byte + 1 of dword g, 0 for an empty dword
__device__ __forceinline__ int alng_len(u32 w, int g) { return w ? 4 * g + 4 - (__clz(w) >> 3) : 0; }

// a - b, 0 where b > a
__device__ __forceinline__ u32 alng_sat(u32 a, u32 b) { return __builtin_elementwise_sub_sat(a, b); }

// the same on both 16-bit halves at once
__device__ __forceinline__ u32 alng_sat2(u32 a, u32 b) {
  return __builtin_bit_cast(u32, __builtin_elementwise_sub_sat(__builtin_bit_cast(alng_u16x2, a), __builtin_bit_cast(alng_u16x2, b)));
}

// One strip of one Y row against the lane's X sequence.  Q: the strip's profile; j0: its first column - 1; jl: the local
// index of len y in the last strip of a global row (else 0); carry_out: write the boundary column for the next strip.
// Returns H[lx][len y] (global, last strip) or the running maximum (local).
template <bool LOCAL, int NC>
__device__ __forceinline__ u32 alng_strip(const unsigned char *Q, const u32 *xb, u32 *wsb, int lane, long long xnpad, int lx, int lxmax,
                                          int j0, int jl, bool carry_out, u32 e, u32 o, u32 bias, u32 best) {
  const u32 oe = o + e, K = oe | (e << 16);
  u32 P[16 * NC + 1];                                                     // P[j] = H[j0 + j] | E[j0 + j] << 16; P[0]: H alone
  if (LOCAL) {
#pragma unroll
    for (int j = 0; j <= 16 * NC; ++j) P[j] = 0;
  } else {
    const u32 b = o + (u32)j0 * e;                                        // H[0][j0], j0 > 0
    P[0] = j0 ? b : 0u;
#pragma unroll
    for (int j = 1; j <= 16 * NC; ++j) P[j] = (b + (u32)j * e) | ((b + o + (u32)j * e) << 16);
  }
  u32 xw = 0, h0 = o;
  for (int i = 0; i < lxmax; ++i) {
    if ((i & 3) == 0) xw = (xb + (long long)(i >> 2) * xnpad)[lane];          // wave-uniform branch and base, coalesced load
    const u32 x = (xw >> (8 * (i & 3))) & 31u;
    h0 += e;                                                              // global: H[i + 1][0] = o + (i + 1) e
    if (i < lx) {
      const unsigned char *q = Q + x * ALN_QSTRIDE;
      u32 *bd = wsb + (long long)i * ALN_THREADS;                         // this step's line of the boundary column
      u32 left, F;
      if (j0) {                                                           // wave-uniform
        const u32 v = bd[lane];
        left = v & 0xffffu;
        F = v >> 16;
      } else {
        left = LOCAL ? 0u : h0;
        F = LOCAL ? 0u : h0 + o;                                          // F[i][0]: -inf clamped | what infinity would give
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
        if (LOCAL) {
#pragma unroll
          for (int t = 0; t < 16; ++t) T[t] = alng_sat(T[t], bias);
        }
        diag = P[16 * c + 16];
#pragma unroll
        for (int t = 0; t < 16; t += 2) {
          u32 h[2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            if (LOCAL) {
              const u32 s = alng_sat2(P[16 * c + t + u + 1], K);          // H -sat- (o + e) | (E -sat- e) << 16
              const u32 E = max(s & 0xffffu, s >> 16);
              F = max(alng_sat(F, e), alng_sat(left, oe));
              left = max(T[t + u], max(E, F));
              P[16 * c + t + u + 1] = left | (E << 16);
            } else {
              const u32 s = P[16 * c + t + u + 1] + K;                    // H + o + e | (E + e) << 16
              const u32 E = min(s & 0xffffu, s >> 16);
              F = min(F + e, left + oe);
              left = min(T[t + u], min(E, F));
              P[16 * c + t + u + 1] = left | (E << 16);
            }
            h[u] = left;
          }
          if (LOCAL) best = max(max(best, h[0]), h[1]);
        }
      }
      if (carry_out) bd[lane] = left | (F << 16);                         // H[i + 1][j0 + 128] | F[i + 1][j0 + 128] << 16
    }
  }
  if (LOCAL) return best;
  u32 res = 0;                                                            // H[len y], 16 (NC - 1) < jl <= 16 NC, jl wave-uniform
#pragma unroll
  for (int t = 1; t <= 16; ++t)
    if (jl == 16 * (NC - 1) + t) res = P[16 * (NC - 1) + t];
  return res & 0xffffu;
}

template <bool LOCAL, typename OUT>
__global__ __launch_bounds__(ALN_THREADS) void pg_aln_long_dense_kernel(
    const u32 *__restrict__ xt, long long n, long long xnpad, int xl, const u32 *__restrict__ yt, long long m, long long ynpad,
    int yl, const unsigned char *__restrict__ table, u32 gap, u32 open, OUT *__restrict__ out, long long ldo, int colTiles,
    int items, u32 *ws) {
  __shared__ __attribute__((aligned(16))) unsigned char Q[ALN_ROWS * ALN_QBYTES];
  __shared__ u32 yrow[ALNG_MAX_L / 4];
  __shared__ unsigned char cs[32 * ALN_CSTRIDE];
  __shared__ int ylen;
  __shared__ int smin;
  const int tid = threadIdx.x;
  const int xg = (xl + 3) >> 2, yg = (yl + 3) >> 2;                         // <= 512 dwords each (the host checks)

  // the table, once per workgroup: costs as they are, scores + bias (bias = -min S >= 0) so that they are bytes
  u32 bias = 0;
  if (LOCAL) {
    if (tid == 0) smin = 0;
    int sc[4], lo = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      sc[k] = (int)(signed char)table[tid + k * ALN_THREADS];
      lo = min(lo, sc[k]);
    }
    __syncthreads();
    if (lo < 0) atomicMin(&smin, lo);
    __syncthreads();
    bias = (u32)(-__builtin_amdgcn_readfirstlane(smin));                   // 0..128, in a scalar register
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = tid + k * ALN_THREADS;
      cs[(i >> 5) * ALN_CSTRIDE + (i & 31)] = (unsigned char)(sc[k] + (int)bias);
    }
  } else {
    for (int i = tid; i < 1024; i += ALN_THREADS) cs[(i >> 5) * ALN_CSTRIDE + (i & 31)] = table[i];
  }

  u32 *wsb = ws + (long long)blockIdx.x * (xg * 4 * ALN_THREADS);          // this workgroup's boundary column
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const long long ct = item % colTiles, row0 = (long long)(item / colTiles) * ALN_ROWS;
    // column ct * 256 + tid (< colTiles * 256 <= xnpad): a wave-uniform base and the lane, so that one VGPR addresses the
    // tokens, the boundary column and the output
    const u32 *xb = xt + ct * ALN_THREADS;
    const long long left_cols = n - ct * ALN_THREADS;                       // >= 1
    int lx = 0;
    for (int g = 0; g < xg; ++g) lx = max(lx, alng_len((xb + (long long)g * xnpad)[tid], g));
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
        if (w) atomicMax(&ylen, alng_len(w, g));
      }
      __syncthreads();
      const int ly = __builtin_amdgcn_readfirstlane(ylen);
      const int ns = (ly + ALN_STRIP - 1) / ALN_STRIP;                    // strips that hold a position of the row
      u32 d = LOCAL ? 0u : (lx ? open + (u32)lx * gap : 0u);              // len y = 0: one run of lx symbols, or nothing
      u32 best = 0;
      for (int s0 = 0; s0 < ns; s0 += ALN_ROWS) {
        const int nb = min(ALN_ROWS, ns - s0);
        if (s0) __syncthreads();                                          // the previous eight strips' profiles are read
        for (int i = tid; i < nb * 32 * 32; i += ALN_THREADS) {
          const int g = i & 31, a = (i >> 5) & 31, slot = i >> 10;
          const int gy = (s0 + slot) * (ALN_STRIP / 4) + g;               // < 512
          const u32 w = yrow[gy];
          const unsigned char *crow = cs + a * ALN_CSTRIDE;               // the table is symmetric: C[a][y] = C[y][a]
          u32 v = (u32)crow[w & 31u] | ((u32)crow[(w >> 8) & 31u] << 8) | ((u32)crow[(w >> 16) & 31u] << 16) |
                  ((u32)crow[(w >> 24) & 31u] << 24);
          if (LOCAL) {
            const int keep = ly - 4 * gy;                                 // positions of this dword inside the sequence
            v &= keep >= 4 ? 0xffffffffu : keep <= 0 ? 0u : (1u << (8 * keep)) - 1u;      // past len y: byte 0, a score of -bias
          }
          *(u32 *)(Q + slot * ALN_QBYTES + a * ALN_QSTRIDE + 4 * g) = v;
        }
        __syncthreads();
        for (int s = s0; s < s0 + nb; ++s) {
          const unsigned char *q = Q + (s - s0) * ALN_QBYTES;
          const bool last = s == ns - 1;
          const int j0 = s * ALN_STRIP, jl = last ? ly - j0 : 0;
          u32 v;
#define ALNG_STRIP(NC) alng_strip<LOCAL, NC>(q, xb, wsb, tid, xnpad, lx, lxmax, j0, LOCAL ? 0 : jl, !last, gap, open, bias, best)
          switch (last ? (jl + 15) >> 4 : 8) {
            case 1: v = ALNG_STRIP(1); break;
            case 2: v = ALNG_STRIP(2); break;
            case 3: v = ALNG_STRIP(3); break;
            case 4: v = ALNG_STRIP(4); break;
            case 5: v = ALNG_STRIP(5); break;
            case 6: v = ALNG_STRIP(6); break;
            case 7: v = ALNG_STRIP(7); break;
            default: v = ALNG_STRIP(8); break;
          }
#undef ALNG_STRIP
          if (LOCAL) best = v;
          else if (last) d = v;
        }
      }
      if (LOCAL) d = best;
      if (tid < left_cols) (out + row * ldo + ct * ALN_THREADS)[tid] = (OUT)d;
    }
  }
}

template <bool LOCAL>
static int alng_launch(const char *name, const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                       int64_t y_npad, int yl, const void *table, int gap, int gap_open, void *out, int64_t ldo, int out_elem_bytes,
                       void *workspace, int64_t workspace_bytes, void *stream) {
  char msg[128];
#define ALNG_FAIL(code, what)                          \
  do {                                                 \
    snprintf(msg, sizeof(msg), "%s: %s", name, what);  \
    return pg_fail(code, msg);                         \
  } while (0)
  if (!x_packed || !y_packed || !table || !out || !workspace || n <= 0 || m <= 0 || xl <= 0 || yl <= 0 || ldo < n)
    ALNG_FAIL(PG_E_BADARG, "bad argument");
  if (xl > ALNG_MAX_L || yl > ALNG_MAX_L) ALNG_FAIL(PG_E_TOOLONG, "at most 2048 positions");
  if (gap < 1 || gap > 255) ALNG_FAIL(PG_E_BADARG, "gap must be in 1..255");
  if (gap_open < 0 || gap_open > 255) ALNG_FAIL(PG_E_BADARG, "gap_open must be in 0..255");
  if (x_npad < n || x_npad % 256 || y_npad < m) ALNG_FAIL(PG_E_BADARG, "bad npad");
  if (out_elem_bytes != 4 && out_elem_bytes != 8) ALNG_FAIL(PG_E_BADARG, "out_elem_bytes must be 4 (int32) or 8");
  const long long one = (long long)ALN_THREADS * (((xl + 3) / 4) * 4) * 4;
  if (workspace_bytes < one) ALNG_FAIL(PG_E_BADARG, "the workspace is smaller than one workgroup's share");
  const long long colTiles = (n + ALN_THREADS - 1) / ALN_THREADS;
  const long long items = colTiles * ((m + ALN_ROWS - 1) / ALN_ROWS);
  long long blocks = workspace_bytes / one;                                 // as many workgroups as the workspace holds
  if (items > 0x7fffffffll) ALNG_FAIL(PG_E_BADARG, "too many pairs for one launch");
  if (blocks > items) blocks = items;
#undef ALNG_FAIL
  const dim3 grid((unsigned)blocks), block(ALN_THREADS);
  if (out_elem_bytes == 4)
    pg_aln_long_dense_kernel<LOCAL, int><<<grid, block, 0, (hipStream_t)stream>>>(
        (const u32 *)x_packed, n, x_npad, xl, (const u32 *)y_packed, m, y_npad, yl, (const unsigned char *)table, (u32)gap,
        (u32)gap_open, (int *)out, ldo, (int)colTiles, (int)items, (u32 *)workspace);
  else
    pg_aln_long_dense_kernel<LOCAL, long long><<<grid, block, 0, (hipStream_t)stream>>>(
        (const u32 *)x_packed, n, x_npad, xl, (const u32 *)y_packed, m, y_npad, yl, (const unsigned char *)table, (u32)gap,
        (u32)gap_open, (long long *)out, ldo, (int)colTiles, (int)items, (u32 *)workspace);
  return pg_launched(name);
}

extern "C" {

int pg_alignment_long_workspace(int xl, int64_t *one_workgroup_bytes, int64_t *full_bytes) {
  if (xl <= 0 || (!one_workgroup_bytes && !full_bytes)) return pg_fail(PG_E_BADARG, "pg_alignment_long_workspace: bad argument");
  if (xl > ALNG_MAX_L) return pg_fail(PG_E_TOOLONG, "pg_alignment_long_workspace: at most 2048 positions");
  const int64_t one = (int64_t)ALN_THREADS * (((xl + 3) / 4) * 4) * 4;
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
  return alng_launch<false>("pg_alignment_long_dense", x_packed, n, x_npad, xl, y_packed, m, y_npad, yl, cost_u8, gap, gap_open, out,
                            ldo, out_elem_bytes, workspace, workspace_bytes, stream);
}

int pg_alignment_local_long_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                                  int64_t y_npad, int yl, const int8_t *score_i8, int gap, int gap_open, void *out, int64_t ldo,
                                  int out_elem_bytes, void *workspace, int64_t workspace_bytes, void *stream) {
  return alng_launch<true>("pg_alignment_local_long_dense", x_packed, n, x_npad, xl, y_packed, m, y_npad, yl, score_i8, gap, gap_open,
                           out, ldo, out_elem_bytes, workspace, workspace_bytes, stream);
}

}  // extern "C"
