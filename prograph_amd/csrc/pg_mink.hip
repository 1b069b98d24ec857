// Minkowski (p = 2) distances of fp16 embeddings and the epsilon / kNN selection on them
// (SURVEY.md §8 f2): the reference's `build_graph(representation="Embedded", distance=minkowski)`
// (prograph/distance/minkowski.py:8-41 through prograph/prograph.py:726-764).
//
// The reference stages the embedding as fp16 (`torch.as_tensor(..., dtype=float16)`, :726) and then
// evaluates  pow(sum(pow(X - Y[:,None,:], 2), axis=2), 1/2)  with fp16 tensors: EVERY elementwise
// step rounds to fp16 (the difference, its square, the sum, the root - and 1/(1+d) twice for
// similarities); only the sum itself accumulates wider.  Its own tests pin that rounding
// (tests/tests.py:164-167: sqrt(0.625) -> 0.79052734).  The kernel reproduces the same sequence:
//     diff = v_pk_add_f16(x, -y)        rounded to fp16, two elements per instruction
//     sq   = v_pk_mul_f16(diff, diff)   rounded to fp16
//     acc += sq.lo + sq.hi              v_dot2c_f32_f16 against (1, 1): exact products, fp32 accumulation in
//                                       element order like the reference's float accumulator (whose own
//                                       order is implementation defined: torch vectorises it)
//     d    = fp16(sqrt(float(fp16(acc))))
// so distances are bit-identical to the reference on the goldens up to D = 64 and differ by one fp16 ulp
// on < 0.05 % of the pairs at D = 1280 (measured against reference-generated goldens, tests/golden/minkowski_f16.npz).
// This is why the ||x||^2 + ||y||^2 - 2 x.y form on the matrix cores is NOT used: it is ~10x cheaper at
// large D but does not round like the reference.
//
// What pins the values beyond those three data sets is an INTERVAL MODEL (tests/minkowski_model.py,
// tests/test_minkowski_values_gpu.py): difference and square are single correctly rounded fp16 operations, so the
// exact sum S of the squares is an integer multiple of 2^-24; any sequence of fp32 additions of these D
// non-negative terms lands within g*S of it, g = D*2^-24 / (1 - D*2^-24), and exactly on it when S = 0 or
// S < 2^24 * (lowest set bit of the terms) - every partial sum of every order is then an fp32 value (integer
// data, near-duplicates whose squares are fp16 subnormals, which the packed fp16 ops and the dot keep).  The two
// ends round to the same or to adjacent fp16 values; each pair's result must be the finish of one of them, which
// for most pairs is bit equality.  The accumulation ORDER is deliberately left free: the model holds for the
// kernel's, for torch's and for the reference's alike, at every D (partial chunks, partial segments, both sides
// of the staged switch) and scale (subnormal squares up to sums on the 65504 | inf boundary).
//
// Layout: embeddings are packed chunk-major like the token planes: chunk q (8 halfs, 16 bytes) of
// vector n at byte (q * Npad + n) * 16, so 64 consecutive vectors load one chunk each as a coalesced
// 1 KiB global_load_dwordx4.
#include "pg_select.h"

#include <hip/hip_fp16.h>

typedef _Float16 pg_h2 __attribute__((ext_vector_type(2)));

#define MK_ROWS 16          // rows (Y vectors) per workgroup of the dense kernel
#define MK_SEG 16           // chunks staged per segment: 128 halfs of every row in LDS

__global__ __launch_bounds__(256) void pg_pack_f16_kernel(const __half *__restrict__ src, long long n, int d, long long ld,
                                                          const long long *__restrict__ rows, uint4 *__restrict__ out,
                                                          long long npad, int nq) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= npad) return;
  const __half *row = s < n ? src + (rows ? rows[s] : s) * ld : nullptr;
  for (int q = 0; q < nq; ++q) {
    union { uint4 v; __half h[8]; } u;
    u.v = make_uint4(0, 0, 0, 0);
    if (row) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int pos = q * 8 + j;
        if (pos < d) u.h[j] = row[pos];
      }
    }
    out[(long long)q * npad + s] = u.v;
  }
}

// ---- the per-pair arithmetic, shared by the dense kernel and the fused graph kernels -------------------------
// one 16-byte chunk (8 halfs) of a pair: difference and square rounded to fp16 two elements per instruction,
// fp32 accumulation in element order (fdot2 against (1, 1): exact products)
__device__ __forceinline__ float mk_chunk(float acc, uint4 xv, uint4 yv) {
  const pg_h2 ones = {(_Float16)1.0f, (_Float16)1.0f};
  const pg_h2 d0 = __builtin_bit_cast(pg_h2, xv.x) - __builtin_bit_cast(pg_h2, yv.x);
  const pg_h2 d1 = __builtin_bit_cast(pg_h2, xv.y) - __builtin_bit_cast(pg_h2, yv.y);
  const pg_h2 d2 = __builtin_bit_cast(pg_h2, xv.z) - __builtin_bit_cast(pg_h2, yv.z);
  const pg_h2 d3 = __builtin_bit_cast(pg_h2, xv.w) - __builtin_bit_cast(pg_h2, yv.w);
  float p = __builtin_amdgcn_fdot2(d0 * d0, ones, acc, false);
  p = __builtin_amdgcn_fdot2(d1 * d1, ones, p, false);
  p = __builtin_amdgcn_fdot2(d2 * d2, ones, p, false);
  return __builtin_amdgcn_fdot2(d3 * d3, ones, p, false);
}

// the accumulated sum -> fp16 distance bits (or similarity 1/(1+d))
__device__ __forceinline__ unsigned short mk_finish(float acc, int similarity) {
  const _Float16 s16 = (_Float16)acc;                               // the float sum as fp16
  __half d16 = __float2half_rn(sqrtf((float)s16));                  // pow(., 1/2) on the fp16 value
  if (similarity) {                                                 // 1 / (1 + d): two fp16 roundings (minkowski.py:40)
    const __half t = __float2half_rn(1.0f + __half2float(d16));
    d16 = __float2half_rn(1.0f / __half2float(t));
  }
  return __half_as_ushort(d16);
}

// acc[r] = sum over all chunks of Y row r (staged in ybuf) against column c of X.  Y rows go through LDS one
// segment of MK_SEG chunks at a time: the thread stages chunk (tid % MK_SEG) of row (tid / MK_SEG), whose Y
// index is `yrow` (< 0: a row past the end, staged as zeros).  staged != 0: nq <= MK_SEG and ybuf already
// holds the whole rows (the fused kernels load them once).  Chunk order = element order, for every caller.
__device__ __forceinline__ void mk_accumulate(float (&acc)[MK_ROWS], const uint4 *__restrict__ xp, long long xnpad, long long c,
                                              const uint4 *__restrict__ yp, long long ynpad, long long yrow, int nq,
                                              uint4 (*ybuf)[MK_SEG], bool staged) {
#pragma unroll
  for (int r = 0; r < MK_ROWS; ++r) acc[r] = 0.0f;
  for (int q0 = 0; q0 < nq; q0 += MK_SEG) {
    if (!staged) {
      __syncthreads();
      const int rr = threadIdx.x / MK_SEG, qq = threadIdx.x % MK_SEG;     // 16 x 16 = 256 chunks per segment
      uint4 v = make_uint4(0, 0, 0, 0);
      if (yrow >= 0 && q0 + qq < nq) v = yp[(long long)(q0 + qq) * ynpad + yrow];
      ybuf[rr][qq] = v;
      __syncthreads();
    }
    const int qn = nq - q0 < MK_SEG ? nq - q0 : MK_SEG;
    for (int qq = 0; qq < qn; ++qq) {
      const uint4 xv = xp[(long long)(q0 + qq) * xnpad + c];
#pragma unroll
      for (int r = 0; r < MK_ROWS; ++r) acc[r] = mk_chunk(acc[r], xv, ybuf[r][qq]);
    }
  }
}

// (M, N) fp16 distance (or similarity) matrix: out[m * ldo + n] = minkowski2(Y[m], X[n])
__global__ __launch_bounds__(256) void pg_mink_dense_kernel(const uint4 *__restrict__ xp, long long n, long long xnpad,
                                                            const uint4 *__restrict__ yp, long long m, long long ynpad,
                                                            int nq, int similarity, __half *__restrict__ out, long long ldo) {
  __shared__ uint4 ybuf[MK_ROWS][MK_SEG];
  const long long col = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long r0 = (long long)blockIdx.y * MK_ROWS;
  const int nr = (int)((m - r0) < MK_ROWS ? (m - r0) : MK_ROWS);
  const long long c = col < xnpad ? col : xnpad - 1;
  const int srow = threadIdx.x / MK_SEG;
  float acc[MK_ROWS];
  mk_accumulate(acc, xp, xnpad, c, yp, ynpad, srow < nr ? r0 + srow : -1, nq, ybuf, false);
  if (col < n) {
#pragma unroll
    for (int r = 0; r < MK_ROWS; ++r) {
      if (r < nr) out[(r0 + r) * ldo + col] = __ushort_as_half(mk_finish(acc[r], similarity));
    }
  }
}

// sortable 16-bit key of a non-negative fp16 value: ascending distance, or descending similarity
__device__ __forceinline__ u32 mk_key(unsigned short bits, int descending) {
  return descending ? (0xFFFFu - (u32)bits) : (u32)bits;
}

// ranks first .. first+k-1 of every row's (key, column) order (the stable sort of :758-760), one wave per row.
// FLOOR (pg_f16_knn_round, first = 0): only pairs after the row's floor (knn_floor) are candidates, and rows are
// written ldo elements apart; the floor is the previous round's last entry, whose fp16 bits give its key back.
template <bool FLOOR>
__global__ __launch_bounds__(256) void pg_f16_knn_kernel(const unsigned short *__restrict__ dist, long long m, long long n,
                                                         long long ld, int k, int first, int descending, int *__restrict__ idx,
                                                         unsigned short *__restrict__ w, const int *__restrict__ floor_idx,
                                                         const unsigned short *__restrict__ floor_w, long long floor_ld,
                                                         long long ldo) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= m) return;
  const unsigned short *d = dist + row * ld;
  u32 lk = 0xFFFFFFFFu, lc = 0xFFFFFFFFu;                 // lane j = j-th smallest (key, column)
  const int last = first + k - 1;
  u32 tk = 0xFFFFFFFFu, tc = 0xFFFFFFFFu;                 // current entry of lane `last`
  u32 fk = 0, fc = 0;
  if (FLOOR) knn_floor(floor_idx[row * floor_ld], mk_key(floor_w[row * floor_ld], descending), fk, fc);
  for (long long c0 = 0; c0 < n; c0 += 64) {
    const long long c = c0 + lane;
    const u32 key = c < n ? mk_key(d[c], descending) : 0xFFFFFFFFu;
    bool cand = c < n && (key < tk || (key == tk && (u32)c < tc));
    if (FLOOR) cand = cand && knn_after(key, (u32)c, fk, fc);
    knn_insert(lk, lc, tk, tc, __builtin_amdgcn_ballot_w64(cand), key, 0, c0, last);
  }
  if (lane >= first && lane <= last) {
    const long long o = row * (FLOOR ? ldo : (long long)k) + (lane - first);
    idx[o] = lc == 0xFFFFFFFFu ? -1 : (int)lc;
    w[o] = lc == 0xFFFFFFFFu ? 0 : d[lc];
  }
}

// epsilon selection (pg_match) on a distance / similarity block: count, or fill at indptr
__global__ __launch_bounds__(256) void pg_f16_eps_kernel(const __half *__restrict__ dist, long long m, long long n, long long ld,
                                                         int cmp, float eps, int similarity, u32 *__restrict__ counts,
                                                         const long long *__restrict__ indptr, int *__restrict__ indices,
                                                         __half *__restrict__ weights) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= m) return;
  const __half *d = dist + row * ld;
  long long run = indptr ? indptr[row] : 0;
  u32 cnt = 0;
  for (long long c0 = 0; c0 < n; c0 += 64) {
    const long long c = c0 + lane;
    const __half v = c < n ? d[c] : __float2half(0.0f);
    const bool hit = c < n && pg_match(__half2float(v), eps, cmp, similarity);
    const u64 mask = __builtin_amdgcn_ballot_w64(hit);
    if (indptr && hit) {
      const long long o = run + mask_rank(mask);
      indices[o] = (int)c;
      weights[o] = v;
    }
    run += __popcll(mask);
    cnt += (u32)__popcll(mask);
  }
  if (!indptr && lane == 0) counts[row] = cnt;
}

// ---- fused distance + selection: no (M, N) block in HBM -----------------------------------------------------
// A workgroup owns MK_ROWS rows (Y vectors) and sweeps all N columns in tiles of MK_TILE: each thread computes its
// column's distances to the 16 rows with the dense kernel's arithmetic (mk_accumulate / mk_finish), the tile's fp16
// values go to LDS, then wave w selects for rows 4w .. 4w+3 from the tile, 64 columns per ballot.  Rows of the
// D <= 128 embeddings are staged in LDS once per workgroup, longer ones one segment at a time per tile.
#define MK_TILE 256
#define MK_RPW (MK_ROWS / 4)      // rows per wave in the selection

// Y index of the row this thread stages: rows r0 .. r0+15, or row_list[g*16 .. g*16+15] (restricted sweeps);
// -1 past the end
__device__ __forceinline__ long long mk_group_row(int rr, long long m, const long long *__restrict__ row_list, long long n_list) {
  const long long g = (long long)blockIdx.x * MK_ROWS + rr;
  if (!row_list) return g < m ? g : -1;
  if (g >= n_list) return -1;
  const long long r = row_list[g];
  return r >= 0 && r < m ? r : -1;
}

// one 256-column tile of the group's fp16 values into LDS: tile[r][j] = value of row r, column t0 + j
__device__ __forceinline__ void mk_tile(unsigned short (*tile)[MK_TILE], const uint4 *__restrict__ xp, long long xnpad, long long t0,
                                        const uint4 *__restrict__ yp, long long ynpad, long long yrow, int nq, uint4 (*ybuf)[MK_SEG],
                                        bool staged, int similarity) {
  float acc[MK_ROWS];
  mk_accumulate(acc, xp, xnpad, t0 + threadIdx.x, yp, ynpad, yrow, nq, ybuf, staged);   // t0 + 255 < xnpad: npad % 256 == 0
  __syncthreads();                                                   // the previous tile's selection is done
#pragma unroll
  for (int r = 0; r < MK_ROWS; ++r) tile[r][threadIdx.x] = mk_finish(acc[r], similarity);
  __syncthreads();
}

__device__ __forceinline__ void mk_stage_once(uint4 (*ybuf)[MK_SEG], const uint4 *__restrict__ yp, long long ynpad, long long yrow,
                                              int nq) {
  const int rr = threadIdx.x / MK_SEG, qq = threadIdx.x % MK_SEG;
  uint4 v = make_uint4(0, 0, 0, 0);
  if (yrow >= 0 && qq < nq) v = yp[(long long)qq * ynpad + yrow];
  ybuf[rr][qq] = v;
  __syncthreads();
}

// ranks first .. first+k-1 of every row's (key, column) order over all n columns: pg_f16_knn on the fly.
// FLOOR (pg_minkowski_knn_round, first = 0): only pairs after each row's floor, rows written ldo elements apart.
template <bool FLOOR>
__global__ __launch_bounds__(256) void pg_mink_knn_kernel(const uint4 *__restrict__ xp, long long n, long long xnpad,
                                                          const uint4 *__restrict__ yp, long long m, long long ynpad, int nq,
                                                          int similarity, int k, int first, int *__restrict__ idx,
                                                          unsigned short *__restrict__ w, const int *__restrict__ floor_idx,
                                                          const unsigned short *__restrict__ floor_w, long long floor_ld,
                                                          long long ldo) {
  __shared__ uint4 ybuf[MK_ROWS][MK_SEG];
  __shared__ unsigned short tile[MK_ROWS][MK_TILE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * MK_ROWS;
  const int nr = (int)((m - r0) < MK_ROWS ? (m - r0) : MK_ROWS);
  const long long yrow = mk_group_row(threadIdx.x / MK_SEG, m, nullptr, 0);
  const bool staged = nq <= MK_SEG;
  if (staged) mk_stage_once(ybuf, yp, ynpad, yrow, nq);
  const int last = first + k - 1;
  u32 lk[MK_RPW], lc[MK_RPW], tk[MK_RPW], tc[MK_RPW];      // lane j = j-th smallest (key, column); entry of lane `last`
#pragma unroll
  for (int j = 0; j < MK_RPW; ++j) lk[j] = lc[j] = tk[j] = tc[j] = 0xFFFFFFFFu;
  u32 fk[MK_RPW], fc[MK_RPW];                                        // the rows' floors (wave-uniform)
#pragma unroll
  for (int j = 0; j < MK_RPW; ++j) {
    fk[j] = fc[j] = 0;
    const long long row = r0 + wv * MK_RPW + j;
    if (FLOOR && row < m) knn_floor(floor_idx[row * floor_ld], mk_key(floor_w[row * floor_ld], similarity), fk[j], fc[j]);
  }
  for (long long t0 = 0; t0 < n; t0 += MK_TILE) {
    mk_tile(tile, xp, xnpad, t0, yp, ynpad, yrow, nq, ybuf, staged, similarity);
    const int ncol = (int)(n - t0 < MK_TILE ? n - t0 : MK_TILE);
#pragma unroll
    for (int j = 0; j < MK_RPW; ++j) {
      const int r = wv * MK_RPW + j;
      if (r >= nr) continue;                                         // wave-uniform
      for (int s0 = 0; s0 < ncol; s0 += 64) {
        const int cc = s0 + lane;
        const u32 key = cc < ncol ? mk_key(tile[r][cc], similarity) : 0xFFFFFFFFu;
        const u32 col = (u32)(t0 + cc);
        bool cand = cc < ncol && (key < tk[j] || (key == tk[j] && col < tc[j]));
        if (FLOOR) cand = cand && knn_after(key, col, fk[j], fc[j]);
        knn_insert(lk[j], lc[j], tk[j], tc[j], __builtin_amdgcn_ballot_w64(cand), key, 0, t0 + s0, last);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < MK_RPW; ++j) {
    const int r = wv * MK_RPW + j;
    if (r < nr && lane >= first && lane <= last) {
      const long long o = (r0 + r) * (FLOOR ? ldo : (long long)k) + (lane - first);
      const bool none = lc[j] == 0xFFFFFFFFu;
      idx[o] = none ? -1 : (int)lc[j];
      w[o] = none ? 0 : (unsigned short)(similarity ? 0xFFFFu - lk[j] : lk[j]);    // mk_key inverted
    }
  }
}

// epsilon selection in the same sweep.  Slot mode (row_list == NULL): every row's exact match count into counts[],
// its first `cap` matches (ascending columns) into its slot.  Fill mode: the rows of row_list only, every match
// written at indptr[row] (counts from a slot pass, so the segments fit).
__global__ __launch_bounds__(256) void pg_mink_eps_kernel(const uint4 *__restrict__ xp, long long n, long long xnpad,
                                                          const uint4 *__restrict__ yp, long long m, long long ynpad, int nq,
                                                          int similarity, int cmp, float eps, const long long *__restrict__ row_list,
                                                          long long n_list, int cap, int *__restrict__ slot_idx,
                                                          unsigned short *__restrict__ slot_w, u32 *__restrict__ counts,
                                                          const long long *__restrict__ indptr, int *__restrict__ indices,
                                                          unsigned short *__restrict__ weights) {
  __shared__ uint4 ybuf[MK_ROWS][MK_SEG];
  __shared__ unsigned short tile[MK_ROWS][MK_TILE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long yrow = mk_group_row(threadIdx.x / MK_SEG, m, row_list, n_list);
  const bool staged = nq <= MK_SEG;
  if (staged) mk_stage_once(ybuf, yp, ynpad, yrow, nq);
  long long row[MK_RPW], base[MK_RPW];
  u32 cnt[MK_RPW];
#pragma unroll
  for (int j = 0; j < MK_RPW; ++j) {
    row[j] = mk_group_row(wv * MK_RPW + j, m, row_list, n_list);
    base[j] = row[j] < 0 ? 0 : (row_list ? indptr[row[j]] : row[j] * (long long)cap);
    cnt[j] = 0;
  }
  for (long long t0 = 0; t0 < n; t0 += MK_TILE) {
    mk_tile(tile, xp, xnpad, t0, yp, ynpad, yrow, nq, ybuf, staged, similarity);
    const int ncol = (int)(n - t0 < MK_TILE ? n - t0 : MK_TILE);
#pragma unroll
    for (int j = 0; j < MK_RPW; ++j) {
      if (row[j] < 0) continue;                                      // wave-uniform
      const int r = wv * MK_RPW + j;
      for (int s0 = 0; s0 < ncol; s0 += 64) {
        const int cc = s0 + lane;
        const unsigned short v = cc < ncol ? tile[r][cc] : 0;
        const bool hit = cc < ncol && pg_match(__half2float(__ushort_as_half(v)), eps, cmp, similarity);
        const u64 mask = __builtin_amdgcn_ballot_w64(hit);
        if (hit) {
          const long long o = (long long)cnt[j] + mask_rank(mask);
          if (row_list) {
            indices[base[j] + o] = (int)(t0 + cc);
            weights[base[j] + o] = v;
          } else if (o < cap) {
            slot_idx[base[j] + o] = (int)(t0 + cc);
            slot_w[base[j] + o] = v;
          }
        }
        cnt[j] += (u32)__popcll(mask);
      }
    }
  }
  if (!row_list && lane == 0) {
#pragma unroll
    for (int j = 0; j < MK_RPW; ++j)
      if (row[j] >= 0) counts[row[j]] = cnt[j];
  }
}

extern "C" {

int pg_f16_nchunks(int d) { return d <= 0 ? 1 : (d + 7) / 8; }

int pg_pack_f16(const void *src, int64_t n, int d, int64_t ld, const int64_t *rows, void *packed, int64_t npad, void *stream) {
  if (!src || !packed || n < 0 || d <= 0 || ld < d) return pg_fail(PG_E_BADARG, "pg_pack_f16: bad argument");
  if (npad < n || npad % 256) return pg_fail(PG_E_BADARG, "pg_pack_f16: npad must be pg_npad(n)");
  pg_pack_f16_kernel<<<dim3((unsigned)(npad / 256)), dim3(256), 0, (hipStream_t)stream>>>(
      (const __half *)src, n, d, ld, (const long long *)rows, (uint4 *)packed, npad, pg_f16_nchunks(d));
  return pg_launched("pg_pack_f16_kernel");
}

int pg_minkowski_dense(const void *x_packed, int64_t n, int64_t x_npad, const void *y_packed, int64_t m, int64_t y_npad,
                       int d, int similarity, void *out_f16, int64_t ldo, void *stream) {
  if (!x_packed || !y_packed || !out_f16 || n <= 0 || m <= 0 || d <= 0 || ldo < n)
    return pg_fail(PG_E_BADARG, "pg_minkowski_dense: bad argument");
  if (x_npad < n || x_npad % 256 || y_npad < m) return pg_fail(PG_E_BADARG, "pg_minkowski_dense: bad npad");
  if ((m + MK_ROWS - 1) / MK_ROWS > 65535) return pg_fail(PG_E_BADARG, "pg_minkowski_dense: m too large for one launch");
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)((m + MK_ROWS - 1) / MK_ROWS));
  pg_mink_dense_kernel<<<grid, dim3(256), 0, (hipStream_t)stream>>>((const uint4 *)x_packed, n, x_npad, (const uint4 *)y_packed, m,
                                                                    y_npad, pg_f16_nchunks(d), similarity ? 1 : 0,
                                                                    (__half *)out_f16, ldo);
  return pg_launched("pg_mink_dense_kernel");
}

int pg_f16_knn(const void *dist_f16, int64_t m, int64_t n, int64_t ld, int k, int first, int descending, int32_t *idx_out,
               void *w_out_f16, void *stream) {
  if (!dist_f16 || !idx_out || !w_out_f16 || m <= 0 || n <= 0 || ld < n) return pg_fail(PG_E_BADARG, "pg_f16_knn: bad argument");
  if (k < 1 || first < 0 || first + k > 64) return pg_fail(PG_E_BADARG, "pg_f16_knn: first + k must be at most 64");
  pg_f16_knn_kernel<false><<<dim3((unsigned)((m + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(
      (const unsigned short *)dist_f16, m, n, ld, k, first, descending ? 1 : 0, idx_out, (unsigned short *)w_out_f16, nullptr,
      nullptr, 0, k);
  return pg_launched("pg_f16_knn_kernel");
}

int pg_f16_knn_round(const void *dist_f16, int64_t m, int64_t n, int64_t ld, int k, int descending, const int32_t *floor_idx,
                     const void *floor_w_f16, int64_t floor_ld, int32_t *idx_out, void *w_out_f16, int64_t ldo, void *stream) {
  if (!dist_f16 || !idx_out || !w_out_f16 || !floor_idx || !floor_w_f16 || m <= 0 || n <= 0 || ld < n || floor_ld < 0 ||
      ldo < k)
    return pg_fail(PG_E_BADARG, "pg_f16_knn_round: bad argument");
  if (k < 1 || k > 64) return pg_fail(PG_E_BADARG, "pg_f16_knn_round: k must be 1..64");
  pg_f16_knn_kernel<true><<<dim3((unsigned)((m + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(
      (const unsigned short *)dist_f16, m, n, ld, k, 0, descending ? 1 : 0, idx_out, (unsigned short *)w_out_f16, floor_idx,
      (const unsigned short *)floor_w_f16, floor_ld, ldo);
  return pg_launched("pg_f16_knn_kernel(round)");
}

int pg_f16_eps_count(const void *dist_f16, int64_t m, int64_t n, int64_t ld, int cmp, float eps_f16, int similarity,
                     uint32_t *counts, void *stream) {
  if (!dist_f16 || !counts || m <= 0 || n <= 0 || ld < n || pg_cmp_bad(cmp))
    return pg_fail(PG_E_BADARG, "pg_f16_eps_count: bad argument");
  pg_f16_eps_kernel<<<dim3((unsigned)((m + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(
      (const __half *)dist_f16, m, n, ld, cmp, eps_f16, similarity ? 1 : 0, counts, nullptr, nullptr, nullptr);
  return pg_launched("pg_f16_eps_kernel(count)");
}

int pg_f16_eps_fill(const void *dist_f16, int64_t m, int64_t n, int64_t ld, int cmp, float eps_f16, int similarity,
                    const int64_t *indptr, int32_t *indices, void *weights_f16, void *stream) {
  if (!dist_f16 || !indptr || !indices || !weights_f16 || m <= 0 || n <= 0 || ld < n || pg_cmp_bad(cmp))
    return pg_fail(PG_E_BADARG, "pg_f16_eps_fill: bad argument");
  pg_f16_eps_kernel<<<dim3((unsigned)((m + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(
      (const __half *)dist_f16, m, n, ld, cmp, eps_f16, similarity ? 1 : 0, nullptr, (const long long *)indptr, indices,
      (__half *)weights_f16);
  return pg_launched("pg_f16_eps_kernel(fill)");
}

static int mk_operands_bad(const void *xp, int64_t n, int64_t x_npad, const void *yp, int64_t m, int64_t y_npad, int d) {
  return !xp || !yp || n <= 0 || m <= 0 || d <= 0 || x_npad < n || x_npad % 256 || y_npad < m;
}

int pg_minkowski_knn(const void *x_packed, int64_t n, int64_t x_npad, const void *y_packed, int64_t m, int64_t y_npad, int d,
                     int similarity, int k, int first, int32_t *idx_out, void *w_out_f16, void *stream) {
  if (mk_operands_bad(x_packed, n, x_npad, y_packed, m, y_npad, d) || !idx_out || !w_out_f16)
    return pg_fail(PG_E_BADARG, "pg_minkowski_knn: bad argument");
  if (k < 1 || first < 0 || first + k > 64) return pg_fail(PG_E_BADARG, "pg_minkowski_knn: first + k must be at most 64");
  if (n > 0xFFFFFFFFll - 1 || (m + MK_ROWS - 1) / MK_ROWS > 0x7FFFFFFFll)
    return pg_fail(PG_E_BADARG, "pg_minkowski_knn: too many vectors for one launch");
  pg_mink_knn_kernel<false><<<dim3((unsigned)((m + MK_ROWS - 1) / MK_ROWS)), dim3(256), 0, (hipStream_t)stream>>>(
      (const uint4 *)x_packed, n, x_npad, (const uint4 *)y_packed, m, y_npad, pg_f16_nchunks(d), similarity ? 1 : 0, k, first,
      idx_out, (unsigned short *)w_out_f16, nullptr, nullptr, 0, k);
  return pg_launched("pg_mink_knn_kernel");
}

int pg_minkowski_knn_round(const void *x_packed, int64_t n, int64_t x_npad, const void *y_packed, int64_t m, int64_t y_npad,
                           int d, int similarity, int k, const int32_t *floor_idx, const void *floor_w_f16, int64_t floor_ld,
                           int32_t *idx_out, void *w_out_f16, int64_t ldo, void *stream) {
  if (mk_operands_bad(x_packed, n, x_npad, y_packed, m, y_npad, d) || !idx_out || !w_out_f16 || !floor_idx || !floor_w_f16 ||
      floor_ld < 0 || ldo < k)
    return pg_fail(PG_E_BADARG, "pg_minkowski_knn_round: bad argument");
  if (k < 1 || k > 64) return pg_fail(PG_E_BADARG, "pg_minkowski_knn_round: k must be 1..64");
  if (n > 0xFFFFFFFFll - 1 || (m + MK_ROWS - 1) / MK_ROWS > 0x7FFFFFFFll)
    return pg_fail(PG_E_BADARG, "pg_minkowski_knn_round: too many vectors for one launch");
  pg_mink_knn_kernel<true><<<dim3((unsigned)((m + MK_ROWS - 1) / MK_ROWS)), dim3(256), 0, (hipStream_t)stream>>>(
      (const uint4 *)x_packed, n, x_npad, (const uint4 *)y_packed, m, y_npad, pg_f16_nchunks(d), similarity ? 1 : 0, k, 0,
      idx_out, (unsigned short *)w_out_f16, floor_idx, (const unsigned short *)floor_w_f16, floor_ld, ldo);
  return pg_launched("pg_mink_knn_kernel(round)");
}

int pg_minkowski_eps_slots(const void *x_packed, int64_t n, int64_t x_npad, const void *y_packed, int64_t m, int64_t y_npad,
                           int d, int similarity, int cmp, float eps_f16, int cap, int32_t *slot_idx, void *slot_w_f16,
                           uint32_t *counts, void *stream) {
  if (mk_operands_bad(x_packed, n, x_npad, y_packed, m, y_npad, d) || !slot_idx || !slot_w_f16 || !counts || cap < 1 ||
      pg_cmp_bad(cmp))
    return pg_fail(PG_E_BADARG, "pg_minkowski_eps_slots: bad argument");
  if (n > 0x7FFFFFFFll || (m + MK_ROWS - 1) / MK_ROWS > 0x7FFFFFFFll)
    return pg_fail(PG_E_BADARG, "pg_minkowski_eps_slots: too many vectors for one launch");
  pg_mink_eps_kernel<<<dim3((unsigned)((m + MK_ROWS - 1) / MK_ROWS)), dim3(256), 0, (hipStream_t)stream>>>(
      (const uint4 *)x_packed, n, x_npad, (const uint4 *)y_packed, m, y_npad, pg_f16_nchunks(d), similarity ? 1 : 0, cmp, eps_f16,
      nullptr, 0, cap, slot_idx, (unsigned short *)slot_w_f16, counts, nullptr, nullptr, nullptr);
  return pg_launched("pg_mink_eps_kernel(slots)");
}

int pg_minkowski_eps_compact(int64_t m, int cap, const int32_t *slot_idx, const void *slot_w_f16, const uint32_t *counts,
                             const int64_t *indptr, int32_t *indices, void *weights_f16, void *stream) {
  return pg_eps_compact_launch<unsigned short>("pg_minkowski_eps_compact", m, cap, slot_idx, slot_w_f16, counts, indptr, indices,
                                               weights_f16, stream);
}

int pg_minkowski_eps_fill_rows(const void *x_packed, int64_t n, int64_t x_npad, const void *y_packed, int64_t m, int64_t y_npad,
                               int d, int similarity, int cmp, float eps_f16, const int64_t *row_list, int64_t n_list,
                               const int64_t *indptr, int32_t *indices, void *weights_f16, void *stream) {
  if (mk_operands_bad(x_packed, n, x_npad, y_packed, m, y_npad, d) || !row_list || n_list <= 0 || !indptr || !indices ||
      !weights_f16 || pg_cmp_bad(cmp))
    return pg_fail(PG_E_BADARG, "pg_minkowski_eps_fill_rows: bad argument");
  if (n > 0x7FFFFFFFll || (n_list + MK_ROWS - 1) / MK_ROWS > 0x7FFFFFFFll)
    return pg_fail(PG_E_BADARG, "pg_minkowski_eps_fill_rows: too many vectors for one launch");
  pg_mink_eps_kernel<<<dim3((unsigned)((n_list + MK_ROWS - 1) / MK_ROWS)), dim3(256), 0, (hipStream_t)stream>>>(
      (const uint4 *)x_packed, n, x_npad, (const uint4 *)y_packed, m, y_npad, pg_f16_nchunks(d), similarity ? 1 : 0, cmp, eps_f16,
      (const long long *)row_list, n_list, 1, nullptr, nullptr, nullptr, (const long long *)indptr, indices,
      (unsigned short *)weights_f16);
  return pg_launched("pg_mink_eps_kernel(fill)");
}

}  // extern "C"
