// Substitution-matrix distance of tokenised sequences:  d(y, x) = sum_j C[y_j][x_j]  with a symmetric cost table C of
// at most 32 symbols and entries 0..255 (BUILD DEFINED: the reference has Hamming only, which is C = 1 - I).
//
// The kernel is the query-profile form of striped Smith-Waterman.  A workgroup owns SUB_ROWS = 16 rows of Y and
// builds, per pass of at most SUB_PASS positions, the LDS image
//     P[j][a][r] = C[y_{r,j}][a]          one byte per (position j, symbol a, row r): 512 bytes per position
// so that ONE 16-byte LDS read at (j, x_j) returns the costs of all 16 rows against the symbol a column holds at
// position j.  Every lane owns one X column, sweeps the positions and adds the 16 bytes into packed 16-bit sums:
//     aw += w                 v_pk_add_u16: lanes b0 + 256 b1 and b2 + 256 b3 of the dword, modulo 2^16
//     ao += w >> 8 (packed)   v_pk_lshrrev_b16 + v_pk_add_u16: lanes b1 and b3, exact
// and at the end of the pass  sum b0 = aw - (ao << 8)  modulo 2^16, which is exact because a pass of SUB_PASS <= 257
// positions keeps every sum below 2^16: 3 VALU instructions per 4 pair-positions instead of 4 with byte extraction.
// The sums of a pass are widened when they leave the registers: a pass adds into `out` (32-bit, 64-bit or fp16
// arithmetic), so widths beyond one pass - and beyond 16 bits, L * 255 from L = 258 - accumulate in the output type.
// The image is rebuilt once per pass and reused for up to SUB_TILES tiles of 512 columns.
//
// Bank conflicts of the image read depend on the data: ds_read_b128 is served in groups of 16 lanes over 16 slots of
// 16 bytes, the slot of a read is x_j mod 16, equal symbols broadcast, and two lanes of a group collide only when
// their symbols differ by 16 (an alphabet of 21 symbols has five such pairs).  All lanes of a group read the same
// position, so no swizzle by position separates them.  -DPG_SUB_SPLIT builds the alternative image of two 256-byte
// halves per position (8 rows each, one 8-byte slot per symbol), meant for two conflict-free ds_read_b64; the compiler
// merges them into one ds_read2_b64, which conflicts like the default and is no faster (DESIGN.md §4.14 has the
// counters of both), so it is kept only to reproduce that record.
//
// Operands: the tokens in TRANSPOSED dword order (pg_sub_pack): dword g of sequence c holds positions 4g..4g+3 and
// lives at (g * npad + c) * 4, so the 64 lanes of a wave read 64 consecutive columns as one coalesced load, and a
// column segment of a matrix is the same buffer from dword row a / 4 on.
#include "pg_common.h"
#include "../../include/prograph_hip.h"

#include <hip/hip_fp16.h>

#define SUB_THREADS 512      // one column per thread and tile
#define SUB_ROWS 16          // Y rows per workgroup: the 16 bytes of one image read
#define SUB_PASS 120         // positions per image: 60 KiB, with the staging below within 64 KiB of LDS
#define SUB_TILES 8          // at most this many tiles of SUB_THREADS columns per workgroup and image
#define SUB_MAX_L 2048
#define SUB_CSTRIDE 36       // bytes per row of the staged cost table: rows 9 banks apart, the byte reads of the image
                             // build (32 symbols against one token) fall on 32 different banks

typedef unsigned short pg_us2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void pg_sub_pack_kernel(const unsigned char *__restrict__ tok, long long n, int l, long long ld,
                                                          u32 a, u32 *__restrict__ packed, long long npad, u32 *flags) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= npad) return;
  const int g = blockIdx.y;
  u32 w = 0;
  bool bad = false;
  if (c < n) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int j = 4 * g + t;
      if (j < l) {
        const u32 v = tok[c * ld + j];
        bad |= v >= a;
        w |= v << (8 * t);
      }
    }
  }
  packed[(long long)g * npad + c] = w;
  if (bad) atomicOr(flags, 1u);
}

template <int OB>
__device__ __forceinline__ void sub_store(void *out, long long at, u32 v, bool add) {
  if constexpr (OB == 2) {
    __half *o = (__half *)out + at;
    float f = (float)v;
    if (add) f += __half2float(*o);
    *o = __float2half(f);
  } else if constexpr (OB == 4) {
    int *o = (int *)out + at;
    *o = (add ? *o : 0) + (int)v;
  } else {
    long long *o = (long long *)out + at;
    *o = (add ? *o : 0ll) + (long long)v;
  }
}

template <int OB>
__global__ __launch_bounds__(SUB_THREADS) void pg_sub_dense_kernel(const u32 *__restrict__ xt, long long n, long long xnpad,
                                                                   const u32 *__restrict__ yt, long long m, long long ynpad, int l,
                                                                   const unsigned char *__restrict__ cost, void *out, long long ldo,
                                                                   int accumulate, int tiles, int imageBytes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sub_lds[];
  unsigned char *const P = sub_lds;                        // the image of the pass
  unsigned char *const ytile = sub_lds + imageBytes;       // [position][row]: the Y tokens of the pass, 16 per position
  unsigned char *const cs = ytile + SUB_PASS * SUB_ROWS;   // the cost table, SUB_CSTRIDE bytes per row
  const int tid = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * SUB_ROWS;
  const long long col0 = (long long)blockIdx.y * tiles * SUB_THREADS;

  for (int i = tid; i < 1024; i += SUB_THREADS) cs[(i >> 5) * SUB_CSTRIDE + (i & 31)] = cost[i];

  for (int p0 = 0; p0 < l; p0 += SUB_PASS) {
    const int pw = min(SUB_PASS, l - p0), gw = (pw + 3) >> 2, g0 = p0 >> 2;
    __syncthreads();                                       // the previous pass has read its image (first pass: nothing)
    for (int i = tid; i < gw * SUB_ROWS; i += SUB_THREADS) {
      const int r = i & (SUB_ROWS - 1), g = i >> 4;
      const u32 w = row0 + r < m ? yt[(long long)(g0 + g) * ynpad + row0 + r] : 0u;
#pragma unroll
      for (int t = 0; t < 4; ++t) ytile[(4 * g + t) * SUB_ROWS + r] = (unsigned char)((w >> (8 * t)) & 31u);
    }
    __syncthreads();
    for (int i = tid; i < gw * 4 * 32; i += SUB_THREADS) {
      const int a = i & 31, j = i >> 5;
      const uint4 y = *(const uint4 *)(ytile + j * SUB_ROWS);
      const unsigned char *crow = cs + a * SUB_CSTRIDE;     // C is symmetric: row a at the tokens = column a of their rows
      const u32 yy[4] = {y.x, y.y, y.z, y.w};
      u32 d[4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        d[q] = j < pw ? (u32)crow[yy[q] & 255u] | ((u32)crow[(yy[q] >> 8) & 255u] << 8) | ((u32)crow[(yy[q] >> 16) & 255u] << 16) |
                            ((u32)crow[yy[q] >> 24] << 24)
                      : 0u;                                 // positions past l in the last dword of the operands: no cost
#ifdef PG_SUB_SPLIT
      *(uint2 *)(P + j * 512 + a * 8) = make_uint2(d[0], d[1]);
      *(uint2 *)(P + j * 512 + 256 + a * 8) = make_uint2(d[2], d[3]);
#else
      *(uint4 *)(P + j * 512 + a * 16) = make_uint4(d[0], d[1], d[2], d[3]);
#endif
    }
    __syncthreads();

    for (int tile = 0; tile < tiles; ++tile) {
      const long long cbase = col0 + (long long)tile * SUB_THREADS;
      if (cbase >= n) break;
      const long long c = cbase + tid;
      const u32 *xp = xt + (long long)g0 * xnpad + (c < xnpad ? c : xnpad - 1);
      pg_us2 aw[4], ao[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) aw[q] = ao[q] = pg_us2{0, 0};
      u32 xw = xp[0];
      for (int g = 0; g < gw; ++g) {
        const u32 xn = g + 1 < gw ? xp[(long long)(g + 1) * xnpad] : 0u;
        const unsigned char *pg = P + g * 2048;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const u32 x = (xw >> (8 * t)) & 31u;
#ifdef PG_SUB_SPLIT
          const uint2 lo = *(const uint2 *)(pg + t * 512 + x * 8), hi = *(const uint2 *)(pg + t * 512 + 256 + x * 8);
          const u32 w[4] = {lo.x, lo.y, hi.x, hi.y};
#else
          const uint4 v = *(const uint4 *)(pg + t * 512 + x * 16);
          const u32 w[4] = {v.x, v.y, v.z, v.w};
#endif
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const pg_us2 ws = __builtin_bit_cast(pg_us2, w[q]);
            aw[q] += ws;
            ao[q] += ws >> 8;
          }
        }
        xw = xn;
      }
      if (c < n) {
        const bool add = accumulate != 0 || p0 > 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const pg_us2 e = aw[q] - (ao[q] << 8);
          const u32 d[4] = {e.x, ao[q].x, e.y, ao[q].y};
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const long long r = row0 + 4 * q + b;
            if (r < m) sub_store<OB>(out, r * ldo + c, d[b], add);
          }
        }
      }
    }
  }
}

extern "C" {

int pg_sub_pack(const uint8_t *tokens, int64_t n, int l, int64_t ld, int a, void *packed, int64_t npad, uint32_t *flags,
                void *stream) {
  if (!tokens || !packed || !flags || n <= 0 || l <= 0 || ld < l || a < 1 || a > 32)
    return pg_fail(PG_E_BADARG, "pg_sub_pack: bad argument");
  if (l > SUB_MAX_L) return pg_fail(PG_E_TOOLONG, "pg_sub_pack: at most 2048 positions");
  if (npad < n || npad % 256) return pg_fail(PG_E_BADARG, "pg_sub_pack: npad must be pg_npad(n)");
  pg_sub_pack_kernel<<<dim3((unsigned)(npad / 256), (unsigned)((l + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(
      tokens, n, l, ld, (u32)a, (u32 *)packed, npad, flags);
  return pg_launched("pg_sub_pack");
}

int pg_substitution_dense(const void *x_packed, int64_t n, int64_t x_npad, const void *y_packed, int64_t m, int64_t y_npad, int l,
                          const uint8_t *cost_u8, void *out, int64_t ldo, int out_elem_bytes, int accumulate, void *stream) {
  if (!x_packed || !y_packed || !cost_u8 || !out || n <= 0 || m <= 0 || l <= 0 || ldo < n)
    return pg_fail(PG_E_BADARG, "pg_substitution_dense: bad argument");
  if (l > SUB_MAX_L) return pg_fail(PG_E_TOOLONG, "pg_substitution_dense: at most 2048 positions");
  if (x_npad < n || x_npad % 256 || y_npad < m) return pg_fail(PG_E_BADARG, "pg_substitution_dense: bad npad");
  if (out_elem_bytes != 2 && out_elem_bytes != 4 && out_elem_bytes != 8)
    return pg_fail(PG_E_BADARG, "pg_substitution_dense: out_elem_bytes must be 2 (fp16), 4 or 8");
  const long long rowBlocks = (m + SUB_ROWS - 1) / SUB_ROWS, ntiles = (n + SUB_THREADS - 1) / SUB_THREADS;
  if (rowBlocks > 0x7fffffffll) return pg_fail(PG_E_BADARG, "pg_substitution_dense: m too large for one launch");
  // tiles per workgroup: as many as amortise the image while the grid still has several workgroups per CU slot
  long long tiles = SUB_TILES;
  while (tiles > 1 && rowBlocks * ((ntiles + tiles - 1) / tiles) < 4096) tiles >>= 1;
  if ((ntiles + tiles - 1) / tiles > 65535) tiles = (ntiles + 65534) / 65535;
  const int pw = l < SUB_PASS ? l : SUB_PASS;
  const int imageBytes = ((pw + 3) / 4) * 4 * 512;
  const size_t lds = (size_t)imageBytes + SUB_PASS * SUB_ROWS + 32 * SUB_CSTRIDE;
  const dim3 grid((unsigned)rowBlocks, (unsigned)((ntiles + tiles - 1) / tiles));
#define SUB_LAUNCH(OB)                                                                                                     \
  pg_sub_dense_kernel<OB><<<grid, dim3(SUB_THREADS), lds, (hipStream_t)stream>>>(                                          \
      (const u32 *)x_packed, n, x_npad, (const u32 *)y_packed, m, y_npad, l, cost_u8, out, ldo, accumulate, (int)tiles, imageBytes)
  if (out_elem_bytes == 2) SUB_LAUNCH(2);
  else if (out_elem_bytes == 4) SUB_LAUNCH(4);
  else SUB_LAUNCH(8);
#undef SUB_LAUNCH
  return pg_launched("pg_substitution_dense");
}

}  // extern "C"
