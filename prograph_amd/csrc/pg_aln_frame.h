// The frame of the gapped-alignment score kernels (pg_aln.hip, pg_aln_affine.hip, pg_aln_local.hip, pg_aln_long.hip,
// pg_aln_semiglobal.hip, pg_aln_fit.hip): everything around the cell loop, once.  DESIGN.md section 4.27.
//
// Shape.  One X sequence per lane, the Y row wave-uniform.  A workgroup of ALN_THREADS columns builds byte query profiles in
// LDS, Q[slot][a][j] = table[a][y_j], ALN_QSTRIDE bytes per symbol, so that one 16-byte LDS read returns the table entries of
// 16 consecutive cells of the DP column, which lives in registers and is indexed at compile time only: the frames switch on
// the wave-uniform chunk count NC = ceil(cells / 16).  ALN_QSTRIDE = 144: the 16-byte slot of a read is (9 a + chunk) mod 16,
// so the lanes of one ds_read_b128 group fall on different slots unless their symbols differ by 16; equal symbols broadcast.
// Operands are in the transposed dword order of pg_sub_pack (dword g of sequence c at (g * npad + c) * 4), column
// ct * 256 + tid addressed as a wave-uniform base plus the lane.  Lengths (last non-zero byte + 1) are found here, from the
// packed dwords: no separate length pass, no host sync.
//
// Two frames.  aln_short_frame (up to ALN_MAX_L positions): the 8 profile slots hold 8 Y rows, the whole row is one strip.
// aln_long_frame (up to ALNG_MAX_L): a workgroup loops over (column tile, row group) items and takes one Y row at a time,
// cut into strips of ALN_STRIP positions, 8 strips to the 8 slots; the left edge of strip s > 0 is the boundary column that
// strip s - 1 wrote to workgroup b's slice of the caller's workspace, one dword per (outer step, lane).  Each has a twin
// whose Y side is a profile operand (aln_short_profile_frame, aln_long_profile_frame; pg_aln_profile.hip).
//
// A mode M is a struct built once per workgroup from AlnParams; it supplies
//     M::SCORE, M::TOP           the table: costs as they are | scores + bias as bytes, with top = max(0, max S) if asked for
//     first(ly, lx)              the result before any cell has run: the answer for an empty y, the initial maximum beyond
//     begin_row(ly)              per-row state (short frame; fit alone has some)
//     row<NC>(q, x, ly)          the short frame's whole row
//     strip<NC, LAST>(q, x, wsb, j0, rest, best)     the long frame's strip j0 / 128; rest = len y - j0 in the last one
//     value<OUT>(d)              the stored result as the output value
#pragma once
#include "pg_common.h"
#include "../../include/prograph_hip.h"

#define ALN_THREADS 256
#define ALN_ROWS 8                 // profile slots: 36 KiB of LDS.  Short: 8 Y rows per workgroup; long: 8 strips of one row
#define ALN_MAX_L 128
#define ALN_STRIP 128
#define ALN_QSTRIDE 144
#define ALN_QBYTES (32 * ALN_QSTRIDE)
#define ALN_CSTRIDE 36             // bytes per row of the staged table (as in pg_sub.hip)
#define ALNG_MAX_L PG_ALN_LONG_MAX_L
#define ALNG_RESIDENT 2            // long kernels, workgroups per CU: 194..198 VGPRs, 2 waves per SIMD (profiles/aln_long_dense.txt)

typedef unsigned short aln_u16x2 __attribute__((ext_vector_type(2)));

// index of the last non-zero byte + 1 of dword g, 0 for an empty dword
__device__ __forceinline__ int aln_len(u32 w, int g) { return w ? 4 * g + 4 - (__clz(w) >> 3) : 0; }

// a - b, 0 where b > a
__device__ __forceinline__ u32 aln_sat(u32 a, u32 b) { return __builtin_elementwise_sub_sat(a, b); }

// the same on both 16-bit halves at once
__device__ __forceinline__ u32 aln_sat2(u32 a, u32 b) {
  return __builtin_bit_cast(u32, __builtin_elementwise_sub_sat(__builtin_bit_cast(aln_u16x2, a), __builtin_bit_cast(aln_u16x2, b)));
}

// NC = 1..8 at compile time; ZERO is the statement for nc == 0 (no cell at all)
#define ALN_NC_SWITCH(nc, ZERO, CALL) \
  switch (nc) {                       \
    case 0: ZERO; break;              \
    case 1: CALL(1); break;           \
    case 2: CALL(2); break;           \
    case 3: CALL(3); break;           \
    case 4: CALL(4); break;           \
    case 5: CALL(5); break;           \
    case 6: CALL(6); break;           \
    case 7: CALL(7); break;           \
    default: CALL(8); break;          \
  }

struct AlnParams {                 // wave-uniform: the kernel's arguments and what the table staging found
  u32 gap, open;
  int xl, yl, obias;
  u32 bias, top;
};

struct AlnX {                      // a lane's X sequence
  const u32 *xb;                   // wave-uniform: dword 0 of the column tile
  long long npad;
  int lane, lx, lxmax;             // its length, the longest of its wave (wave-uniform)
};

// the dword that holds token i (i a multiple of 4 where it is called: a wave-uniform branch, a coalesced load)
__device__ __forceinline__ u32 aln_x_word(const AlnX &x, int i) { return (x.xb + (long long)(i >> 2) * x.npad)[x.lane]; }

// what a mode need not say
struct AlnModeBase {
  __device__ __forceinline__ void begin_row(int) {}
  template <typename OUT>
  __device__ __forceinline__ OUT value(u32 d) const { return (OUT)d; }
};

// the cost table into LDS as it is
__device__ __forceinline__ void aln_cost_table(const unsigned char *cost, unsigned char *cs, int tid) {
  for (int i = tid; i < 1024; i += ALN_THREADS) cs[(i >> 5) * ALN_CSTRIDE + (i & 31)] = cost[i];
}

// the score table into LDS as bytes S + bias; returns bias = -min(0, min S) and, if TOP, *top = max(0, max S), both
// wave-uniform.  Two barriers, the second after every thread's global loads: they cover what the caller staged before.
template <bool TOP>
__device__ __forceinline__ u32 aln_score_table(const signed char *score, unsigned char *cs, int *smin, int *smax, int tid, u32 *top) {
  if (tid == 0) {
    *smin = 0;
    if (TOP) *smax = 0;
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
  if (TOP && hi > 0) atomicMax(smax, hi);
  __syncthreads();
  const u32 bias = (u32)(-__builtin_amdgcn_readfirstlane(*smin));            // 0..128, in a scalar register
  *top = TOP ? (u32)__builtin_amdgcn_readfirstlane(*smax) : 0u;             // 0..127
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = tid + k * ALN_THREADS;
    cs[(i >> 5) * ALN_CSTRIDE + (i & 31)] = (unsigned char)(sc[k] + (int)bias);
  }
  return bias;
}

// four profile bytes of symbol row `crow` against the tokens of dword w (the table is symmetric: T[a][y] = T[y][a]); KEEP:
// positions past the sequence (keep < 4) are byte 0, a score of -bias
template <bool KEEP>
__device__ __forceinline__ u32 aln_profile(const unsigned char *crow, u32 w, int keep) {
  const u32 d = (u32)crow[w & 31u] | ((u32)crow[(w >> 8) & 31u] << 8) | ((u32)crow[(w >> 16) & 31u] << 16) |
                ((u32)crow[(w >> 24) & 31u] << 24);
  return KEEP ? d & (keep >= 4 ? 0xffffffffu : keep <= 0 ? 0u : (1u << (8 * keep)) - 1u) : d;
}

// a lane's length and its wave's longest; column ct * 256 + tid < colTiles * 256 <= xnpad, left_cols = n - ct * 256 >= 1
__device__ __forceinline__ AlnX aln_x(const u32 *xb, long long xnpad, int xg, int tid, long long left_cols) {
  int lx = 0;
  for (int g = 0; g < xg; ++g) lx = max(lx, aln_len((xb + (long long)g * xnpad)[tid], g));
  if (tid >= left_cols) lx = 0;
  int lxmax = lx;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) lxmax = max(lxmax, __shfl_xor(lxmax, s));
  return AlnX{xb, xnpad, tid, lx, __builtin_amdgcn_readfirstlane(lxmax)};
}

// Up to ALN_MAX_L positions: workgroup (ct, rg) owns 256 columns and the ALN_ROWS rows of Y from rg * ALN_ROWS.
template <class M, typename OUT>
__device__ __forceinline__ void aln_short_frame(const u32 *__restrict__ xt, long long n, long long xnpad, int xl,
                                                const u32 *__restrict__ yt, long long m, long long ynpad, int yl,
                                                const void *__restrict__ table, u32 gap, u32 open, int obias, OUT *__restrict__ out,
                                                long long ldo, long long colTiles) {
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
  u32 bias = 0, top = 0;
  if (M::SCORE) {
    bias = aln_score_table<M::TOP>((const signed char *)table, cs, &smin, &smax, tid, &top);      // its barriers cover ytile
  } else {
    aln_cost_table((const unsigned char *)table, cs, tid);
    __syncthreads();
  }
  if (tid < ALN_ROWS) {
    int len = 0;
    for (int g = 0; g < ALN_MAX_L / 4; ++g) len = max(len, aln_len(ytile[tid][g], g));
    ylen[tid] = len;
  }
  if (M::SCORE) __syncthreads();                                            // the masked gather reads ylen
  for (int i = tid; i < ALN_ROWS * 32 * 32; i += ALN_THREADS) {
    const int g = i & 31, a = (i >> 5) & 31, r = i >> 10;
    *(u32 *)(Q + r * ALN_QBYTES + a * ALN_QSTRIDE + 4 * g) =
        aln_profile<M::SCORE>(cs + a * ALN_CSTRIDE, ytile[r][g], M::SCORE ? ylen[r] - 4 * g : 4);
  }
  __syncthreads();

  const long long left_cols = n - ct * ALN_THREADS;
  const AlnX x = aln_x(xt + ct * ALN_THREADS, xnpad, xg, tid, left_cols);
  M mode(AlnParams{gap, open, xl, yl, obias, bias, top});
  for (int r = 0; r < ALN_ROWS; ++r) {
    const long long row = row0 + r;
    if (row >= m) break;
    const int ly = __builtin_amdgcn_readfirstlane(ylen[r]);
    const unsigned char *q = Q + r * ALN_QBYTES;
    mode.begin_row(ly);
    u32 d;
#define ALN_ROW(NC) d = mode.template row<NC>(q, x, ly)
    ALN_NC_SWITCH((ly + 15) >> 4, d = mode.first(0, x.lx), ALN_ROW)
#undef ALN_ROW
    if (tid < left_cols) (out + row * ldo + ct * ALN_THREADS)[tid] = mode.template value<OUT>(d);
  }
}

// Up to ALNG_MAX_L positions: workgroup b loops over its items and owns slice b of the workspace.
template <class M, typename OUT>
__device__ __forceinline__ void aln_long_frame(const u32 *__restrict__ xt, long long n, long long xnpad, int xl,
                                               const u32 *__restrict__ yt, long long m, long long ynpad, int yl,
                                               const void *__restrict__ table, u32 gap, u32 open, int obias, OUT *__restrict__ out,
                                               long long ldo, int colTiles, int items, u32 *ws) {
  __shared__ __attribute__((aligned(16))) unsigned char Q[ALN_ROWS * ALN_QBYTES];
  __shared__ u32 yrow[ALNG_MAX_L / 4];
  __shared__ unsigned char cs[32 * ALN_CSTRIDE];
  __shared__ int ylen;
  __shared__ int smin, smax;
  const int tid = threadIdx.x;
  const int xg = (xl + 3) >> 2, yg = (yl + 3) >> 2;                         // <= 512 dwords each (the host checks)
  u32 bias = 0, top = 0;
  if (M::SCORE) bias = aln_score_table<M::TOP>((const signed char *)table, cs, &smin, &smax, tid, &top);
  else aln_cost_table((const unsigned char *)table, cs, tid);
  const M mode(AlnParams{gap, open, xl, yl, obias, bias, top});

  u32 *wsb = ws + (long long)blockIdx.x * (xg * 4 * ALN_THREADS);          // this workgroup's boundary column
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const long long ct = item % colTiles, row0 = (long long)(item / colTiles) * ALN_ROWS;
    const long long left_cols = n - ct * ALN_THREADS;
    const AlnX x = aln_x(xt + ct * ALN_THREADS, xnpad, xg, tid, left_cols);

    for (int r = 0; r < ALN_ROWS; ++r) {
      const long long row = row0 + r;
      if (row >= m) break;
      __syncthreads();                                                    // the previous row's readers of Q / yrow / ylen are done
      if (tid == 0) ylen = 0;
      __syncthreads();
      for (int g = tid; g < ALNG_MAX_L / 4; g += ALN_THREADS) {
        const u32 w = g < yg ? yt[(long long)g * ynpad + row] : 0u;
        yrow[g] = w;
        if (w) atomicMax(&ylen, aln_len(w, g));
      }
      __syncthreads();
      const int ly = __builtin_amdgcn_readfirstlane(ylen);
      const int ns = (ly + ALN_STRIP - 1) / ALN_STRIP;                    // strips that hold a position of the row
      u32 best = mode.first(ly, x.lx);                                    // carried from strip to strip
      for (int s0 = 0; s0 < ns; s0 += ALN_ROWS) {
        const int nb = min(ALN_ROWS, ns - s0);
        if (s0) __syncthreads();                                          // the previous eight strips' profiles are read
        for (int i = tid; i < nb * 32 * 32; i += ALN_THREADS) {
          const int g = i & 31, a = (i >> 5) & 31, slot = i >> 10;
          const int gy = (s0 + slot) * (ALN_STRIP / 4) + g;               // < 512
          *(u32 *)(Q + slot * ALN_QBYTES + a * ALN_QSTRIDE + 4 * g) = aln_profile<M::SCORE>(cs + a * ALN_CSTRIDE, yrow[gy], ly - 4 * gy);
        }
        __syncthreads();
        for (int s = s0; s < s0 + nb; ++s) {
          const unsigned char *q = Q + (s - s0) * ALN_QBYTES;
          const int j0 = s * ALN_STRIP;
          if (s < ns - 1) {
            best = mode.template strip<8, false>(q, x, wsb, j0, 0, best);
            continue;
          }
          const int rest = ly - j0;                                       // 1..128
#define ALN_LAST(NC) best = mode.template strip<NC, true>(q, x, wsb, j0, rest, best)
          ALN_NC_SWITCH((rest + 15) >> 4, (void)0, ALN_LAST)
#undef ALN_LAST
        }
      }
      if (tid < left_cols) (out + row * ldo + ct * ALN_THREADS)[tid] = mode.template value<OUT>(best);
    }
  }
}

// ---- the profile source (pg_aln_profile.hip): the Y side is a position-specific score matrix, so its
// query profile is not gathered from tokens and a table but copied from global memory.  Frames of their own: the token
// frames above, which sit on the register cliff, stay as they are ----

struct AlnProfiles {               // wave-uniform
  const u32 *p;                    // bytes P + bias, [profile][32 symbols][4 * lpad4 positions]
  const int *len;                  // positions of every profile: lengths are given, never found from bytes
  int lpad4;                       // dwords per symbol row: a multiple of ALN_STRIP / 4 that covers the longest profile
};

// a profile's length as the frames use it: inside the operand, whatever the array holds
__device__ __forceinline__ int aln_profile_len(const AlnProfiles &pf, long long row, int yl, int max_l) {
  return min(max(pf.len[row], 0), min(yl, max_l));
}

// dword g of symbol a of profile `row` (g < lpad4); positions from ly on are byte 0, a score of -bias
__device__ __forceinline__ u32 aln_profile_word(const AlnProfiles &pf, long long row, int a, int g, int ly) {
  const int keep = ly - 4 * g;
  const u32 d = pf.p[(row * 32 + a) * pf.lpad4 + g];
  return d & (keep >= 4 ? 0xffffffffu : keep <= 0 ? 0u : (1u << (8 * keep)) - 1u);
}

// aln_short_frame with 8 profiles in the 8 slots: a coalesced dword copy into the ALN_QSTRIDE rows, no ytile, no table.
// bias = -min(0, min P) and top = max(0, max P) over the call's profiles come from the host.
template <class M, typename OUT>
__device__ __forceinline__ void aln_short_profile_frame(const u32 *__restrict__ xt, long long n, long long xnpad, int xl,
                                                        const AlnProfiles pf, long long m, int yl, u32 gap, u32 open, int obias,
                                                        u32 bias, u32 top, OUT *__restrict__ out, long long ldo, long long colTiles) {
  __shared__ __attribute__((aligned(16))) unsigned char Q[ALN_ROWS * ALN_QBYTES];
  __shared__ int ylen[ALN_ROWS];
  const int tid = threadIdx.x;
  const long long ct = (long long)blockIdx.x % colTiles, rg = (long long)blockIdx.x / colTiles;
  const long long row0 = rg * ALN_ROWS;
  const int xg = (xl + 3) >> 2;                                             // <= 32 dwords (the host checks)

  if (tid < ALN_ROWS) ylen[tid] = row0 + tid < m ? aln_profile_len(pf, row0 + tid, yl, ALN_MAX_L) : 0;
  __syncthreads();
  for (int i = tid; i < ALN_ROWS * 32 * 32; i += ALN_THREADS) {
    const int g = i & 31, a = (i >> 5) & 31, r = i >> 10;                   // a workgroup reads 4 KiB runs: lpad4 = 32 here
    *(u32 *)(Q + r * ALN_QBYTES + a * ALN_QSTRIDE + 4 * g) = row0 + r < m ? aln_profile_word(pf, row0 + r, a, g, ylen[r]) : 0u;
  }
  __syncthreads();

  const long long left_cols = n - ct * ALN_THREADS;
  const AlnX x = aln_x(xt + ct * ALN_THREADS, xnpad, xg, tid, left_cols);
  M mode(AlnParams{gap, open, xl, yl, obias, bias, top});
  for (int r = 0; r < ALN_ROWS; ++r) {
    const long long row = row0 + r;
    if (row >= m) break;
    const int ly = __builtin_amdgcn_readfirstlane(ylen[r]);
    const unsigned char *q = Q + r * ALN_QBYTES;
    mode.begin_row(ly);
    u32 d;
#define ALN_ROW(NC) d = mode.template row<NC>(q, x, ly)
    ALN_NC_SWITCH((ly + 15) >> 4, d = mode.first(0, x.lx), ALN_ROW)
#undef ALN_ROW
    if (tid < left_cols) (out + row * ldo + ct * ALN_THREADS)[tid] = mode.template value<OUT>(d);
  }
}

// aln_long_frame with the 8 strips of one profile in the 8 slots, read straight from global memory: no yrow, no table
template <class M, typename OUT>
__device__ __forceinline__ void aln_long_profile_frame(const u32 *__restrict__ xt, long long n, long long xnpad, int xl,
                                                       const AlnProfiles pf, long long m, int yl, u32 gap, u32 open, int obias,
                                                       u32 bias, u32 top, OUT *__restrict__ out, long long ldo, int colTiles,
                                                       int items, u32 *ws) {
  __shared__ __attribute__((aligned(16))) unsigned char Q[ALN_ROWS * ALN_QBYTES];
  const int tid = threadIdx.x;
  const int xg = (xl + 3) >> 2;                                             // <= 512 dwords (the host checks)
  const M mode(AlnParams{gap, open, xl, yl, obias, bias, top});

  u32 *wsb = ws + (long long)blockIdx.x * (xg * 4 * ALN_THREADS);          // this workgroup's boundary column
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const long long ct = item % colTiles, row0 = (long long)(item / colTiles) * ALN_ROWS;
    const long long left_cols = n - ct * ALN_THREADS;
    const AlnX x = aln_x(xt + ct * ALN_THREADS, xnpad, xg, tid, left_cols);

    for (int r = 0; r < ALN_ROWS; ++r) {
      const long long row = row0 + r;
      if (row >= m) break;
      const int ly = __builtin_amdgcn_readfirstlane(aln_profile_len(pf, row, yl, ALNG_MAX_L));      // <= yl <= 4 * lpad4 (the host checks)
      const int ns = (ly + ALN_STRIP - 1) / ALN_STRIP;                    // strips that hold a position of the profile
      u32 best = mode.first(ly, x.lx);                                    // carried from strip to strip
      for (int s0 = 0; s0 < ns; s0 += ALN_ROWS) {
        const int nb = min(ALN_ROWS, ns - s0);
        __syncthreads();                                                  // the previous eight strips', or profile's, readers are done
        for (int i = tid; i < nb * 32 * 32; i += ALN_THREADS) {
          const int g = i & 31, a = (i >> 5) & 31, slot = i >> 10;
          const int gy = (s0 + slot) * (ALN_STRIP / 4) + g;               // < 32 ns <= lpad4
          *(u32 *)(Q + slot * ALN_QBYTES + a * ALN_QSTRIDE + 4 * g) = aln_profile_word(pf, row, a, gy, ly);
        }
        __syncthreads();
        for (int s = s0; s < s0 + nb; ++s) {
          const unsigned char *q = Q + (s - s0) * ALN_QBYTES;
          const int j0 = s * ALN_STRIP;
          if (s < ns - 1) {
            best = mode.template strip<8, false>(q, x, wsb, j0, 0, best);
            continue;
          }
          const int rest = ly - j0;                                       // 1..128
#define ALN_LAST(NC) best = mode.template strip<NC, true>(q, x, wsb, j0, rest, best)
          ALN_NC_SWITCH((rest + 15) >> 4, (void)0, ALN_LAST)
#undef ALN_LAST
        }
      }
      if (tid < left_cols) (out + row * ldo + ct * ALN_THREADS)[tid] = mode.template value<OUT>(best);
    }
  }
}

// ---- host side: one argument check and one launch per frame ----

struct AlnCall {                   // the arguments of a dense entry; gap_open, bias, ws: 0 where the entry has none
  const void *x;
  int64_t n, x_npad;
  int xl;
  const void *y;
  int64_t m, y_npad;
  int yl;
  const void *table;
  int gap, gap_open, bias;
  void *out;
  int64_t ldo;
  int out_elem_bytes;
  void *ws;
  int64_t ws_bytes;
  void *stream;
};

template <typename OUT>
using AlnShortKernel = void(const u32 *, long long, long long, int, const u32 *, long long, long long, int, const void *, u32, u32, int,
                            OUT *, long long, long long);
template <typename OUT>
using AlnLongKernel = void(const u32 *, long long, long long, int, const u32 *, long long, long long, int, const void *, u32, u32, int,
                           OUT *, long long, int, int, u32 *);

// one workgroup's share of the workspace of the long kernels: a boundary column per lane, xl rounded up to 4
static inline long long aln_long_share(int xl) { return (long long)ALN_THREADS * (((xl + 3) / 4) * 4) * 4; }

// 0, or the error: "<entry name>: <text>".  *items: (column tile, row group) pairs; *blocks: workgroups to launch
static inline int aln_check(const char *name, bool lng, const AlnCall &c, long long *colTiles, long long *items, long long *blocks) {
  char msg[128];
#define ALN_FAIL(code, what)                           \
  do {                                                 \
    snprintf(msg, sizeof(msg), "%s: %s", name, what);  \
    return pg_fail(code, msg);                         \
  } while (0)
  if (!c.x || !c.y || !c.table || !c.out || (lng && !c.ws) || c.n <= 0 || c.m <= 0 || c.xl <= 0 || c.yl <= 0 || c.ldo < c.n)
    ALN_FAIL(PG_E_BADARG, "bad argument");
  const int max_l = lng ? ALNG_MAX_L : ALN_MAX_L;
  if (c.xl > max_l || c.yl > max_l) ALN_FAIL(PG_E_TOOLONG, lng ? "at most 2048 positions" : "at most 128 positions");
  if (c.gap < 1 || c.gap > 255) ALN_FAIL(PG_E_BADARG, "gap must be in 1..255");
  if (c.gap_open < 0 || c.gap_open > 255) ALN_FAIL(PG_E_BADARG, "gap_open must be in 0..255");
  if (c.bias < 0) ALN_FAIL(PG_E_BADARG, "bias must not be negative");
  if (c.x_npad < c.n || c.x_npad % 256 || c.y_npad < c.m) ALN_FAIL(PG_E_BADARG, "bad npad");
  if (c.out_elem_bytes != (lng ? 4 : 2) && c.out_elem_bytes != 8)
    ALN_FAIL(PG_E_BADARG, lng ? "out_elem_bytes must be 4 (int32) or 8" : "out_elem_bytes must be 2 (fp16) or 8");
  const long long one = aln_long_share(c.xl);
  if (lng && c.ws_bytes < one) ALN_FAIL(PG_E_BADARG, "the workspace is smaller than one workgroup's share");
  *colTiles = (c.n + ALN_THREADS - 1) / ALN_THREADS;
  *items = *colTiles * ((c.m + ALN_ROWS - 1) / ALN_ROWS);
  if (*items > 0x7fffffffll) ALN_FAIL(PG_E_BADARG, "too many pairs for one launch");
#undef ALN_FAIL
  *blocks = lng && c.ws_bytes / one < *items ? c.ws_bytes / one : *items;   // long: as many workgroups as the workspace holds
  return 0;
}

// fp16 or int64 out
static inline int aln_launch_short(const char *name, const AlnCall &c, AlnShortKernel<_Float16> *k2, AlnShortKernel<long long> *k8) {
  long long colTiles, items, blocks;
  if (const int rc = aln_check(name, false, c, &colTiles, &items, &blocks)) return rc;
  const dim3 grid((unsigned)blocks), block(ALN_THREADS);
  if (c.out_elem_bytes == 2)
    k2<<<grid, block, 0, (hipStream_t)c.stream>>>((const u32 *)c.x, c.n, c.x_npad, c.xl, (const u32 *)c.y, c.m, c.y_npad, c.yl, c.table,
                                                  (u32)c.gap, (u32)c.gap_open, c.bias, (_Float16 *)c.out, c.ldo, colTiles);
  else
    k8<<<grid, block, 0, (hipStream_t)c.stream>>>((const u32 *)c.x, c.n, c.x_npad, c.xl, (const u32 *)c.y, c.m, c.y_npad, c.yl, c.table,
                                                  (u32)c.gap, (u32)c.gap_open, c.bias, (long long *)c.out, c.ldo, colTiles);
  return pg_launched(name);
}

// int32 or int64 out
static inline int aln_launch_long(const char *name, const AlnCall &c, AlnLongKernel<int> *k4, AlnLongKernel<long long> *k8) {
  long long colTiles, items, blocks;
  if (const int rc = aln_check(name, true, c, &colTiles, &items, &blocks)) return rc;
  const dim3 grid((unsigned)blocks), block(ALN_THREADS);
  if (c.out_elem_bytes == 4)
    k4<<<grid, block, 0, (hipStream_t)c.stream>>>((const u32 *)c.x, c.n, c.x_npad, c.xl, (const u32 *)c.y, c.m, c.y_npad, c.yl, c.table,
                                                  (u32)c.gap, (u32)c.gap_open, c.bias, (int *)c.out, c.ldo, (int)colTiles, (int)items,
                                                  (u32 *)c.ws);
  else
    k8<<<grid, block, 0, (hipStream_t)c.stream>>>((const u32 *)c.x, c.n, c.x_npad, c.xl, (const u32 *)c.y, c.m, c.y_npad, c.yl, c.table,
                                                  (u32)c.gap, (u32)c.gap_open, c.bias, (long long *)c.out, c.ldo, (int)colTiles, (int)items,
                                                  (u32 *)c.ws);
  return pg_launched(name);
}
