// Cosine distance of fp16 embeddings on the matrix cores, and the epsilon / kNN selection on it:
// `build_graph(representation="Embedded", distance=cosine)`.  The reference exports `cosine` but never
// implemented it, so the arithmetic below is this project's own contract:
//
//   p  = sum x_k y_k,  nx = sum x_k^2,  ny = sum y_k^2      fp32, all three from ONE tile routine (cs_tile):
//                                                           v_mfma_f32_32x32x16_f16, exact fp16 products, fp32
//                                                           accumulation, K in chunk order.  nx is the diagonal
//                                                           of a tile of the vectors against themselves
//                                                           (pg_cosine_prep), r = 1/sqrt(n) rounded once each.
//   d  = 1                        if nx == 0 or ny == 0     (a zero vector has cosine 0 with everything)
//      = 0                        if p == nx == ny bitwise  (duplicates and self pairs are exactly 0)
//      = clamp(1 - (p*ry)*rx, 0, 2)                         every step rounded to fp32, nothing contracted
//   s  = 1/(1+d)                  similarity, correctly rounded fp32 quotient
//
// Layout: the pg_pack_f16 buffers of pg_mink.hip.  Chunk q (8 halfs) of vector n sits at byte (q*npad + n)*16,
// and that is one lane's A or B fragment of v_mfma_f32_32x32x16_f16: lane l holds k = 8(l>>5) + j of row /
// column l&31, so step s of the K loop reads chunk 2s + (l>>5) of vector l&31, one coalesced dwordx4 per lane
// and operand, no LDS.  An odd chunk count reads the missing last chunk as zeros.
//
// The 32x32 result has the X column on the lane (l&31) and the Y rows in the 16 registers: register r of lane
// half h is row (r&3) + 8(r>>2) + 4h.  The dense kernel writes it out; the fused kernels select from it in
// registers.  Both call cs_tile and cs_finish, so the fused graphs are exactly the selection over the dense block.
//
// Euclidean distance, `distance=euclidean`, is a second epilogue on the same three sums: every kernel
// below except the norm pass is a template over the epilogue and is instantiated for both metrics, and the pg_euclidean_*
// entries share the pg_cosine_* entries' argument lists, checks and launch code.
#include "pg_select.h"

typedef _Float16 cs_h8 __attribute__((ext_vector_type(8)));
typedef float cs_f16 __attribute__((ext_vector_type(16)));

#define CS_T 32              // rows and columns of one MFMA tile; one wave owns CS_T rows
#define CS_WAVES 4           // waves per workgroup

// Y row of register r in lane half h
__device__ __forceinline__ int cs_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// acc[r] = p of (Y vector yrow of this lane's row slot, X vector xcol of this lane's column) in the tile layout:
// lane l supplies row slot / column l&31 (yrow / xcol < 0: a zero vector).  The K loop runs over chunk pairs in
// ascending order for every caller.
__device__ __forceinline__ cs_f16 cs_tile(const uint4 *__restrict__ xp, long long xnpad, long long xcol,
                                          const uint4 *__restrict__ yp, long long ynpad, long long yrow, int nq) {
  const int h = (threadIdx.x >> 5) & 1;
  cs_f16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll 4
  for (int q0 = 0; q0 < nq; q0 += 2) {
    const int q = q0 + h;
    uint4 a = make_uint4(0, 0, 0, 0), b = make_uint4(0, 0, 0, 0);
    if (q < nq) {
      if (yrow >= 0) a = yp[(long long)q * ynpad + yrow];
      if (xcol >= 0) b = xp[(long long)q * xnpad + xcol];
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(cs_h8, a), __builtin_bit_cast(cs_h8, b), acc, 0, 0, 0);
  }
  return acc;
}

// p and the two vectors' norms -> fp32 distance, or similarity 1/(1+d)  (compiled with -ffp-contract=off)
__device__ __forceinline__ float cs_finish(float p, float nx, float rx, float ny, float ry, int similarity) {
  float d;
  if (nx == 0.0f || ny == 0.0f) {
    d = 1.0f;
  } else if (__float_as_uint(p) == __float_as_uint(nx) && __float_as_uint(p) == __float_as_uint(ny)) {
    d = 0.0f;
  } else {
    const float c = (p * ry) * rx;
    d = fminf(fmaxf(1.0f - c, 0.0f), 2.0f);
  }
  return similarity ? 1.0f / (1.0f + d) : d;
}

// Euclidean epilogue on the same three sums: d = sqrt(max((nx + ny) - (p + p), 0)), every step rounded
// to fp32 and the root correctly rounded; identical vectors (p == nx == ny bitwise, two zero vectors included) are
// exactly 0, and a zero vector is an ordinary point: d(0, y) = sqrt(ny).
__device__ __forceinline__ float eu_finish(float p, float nx, float ny, int similarity) {
  float d;
  if (__float_as_uint(p) == __float_as_uint(nx) && __float_as_uint(p) == __float_as_uint(ny)) {
    d = 0.0f;
  } else {
    d = sqrtf(fmaxf((nx + ny) - (p + p), 0.0f));
  }
  return similarity ? 1.0f / (1.0f + d) : d;
}

// The epilogue of a kernel instance: the dense, kNN and eps kernels below are templates over one of these and share
// everything else.  The Euclidean instances never read the reciprocal roots.
struct cs_cosine {
  static __device__ __forceinline__ float finish(float p, float nx, float rx, float ny, float ry, int similarity) {
    return cs_finish(p, nx, rx, ny, ry, similarity);
  }
};
struct cs_euclid {
  static __device__ __forceinline__ float finish(float p, float nx, float, float ny, float, int similarity) {
    return eu_finish(p, nx, ny, similarity);
  }
};

// sortable key of a non-negative fp32 value: ascending distance, or descending similarity (s > 0: never ~0u)
__device__ __forceinline__ u32 cs_key(float v, int descending) {
  const u32 b = __float_as_uint(v);
  return descending ? ~b : b;
}
__device__ __forceinline__ float cs_unkey(u32 key, int descending) { return __uint_as_float(descending ? ~key : key); }

// ---- per-vector norms: the diagonal of cs_tile on 32 vectors against themselves --------------------------------
__global__ __launch_bounds__(256) void pg_cos_prep_kernel(const uint4 *__restrict__ xp, long long n, long long npad, int nq,
                                                          float *__restrict__ norm, float *__restrict__ rnorm,
                                                          u32 *__restrict__ flags) {
  const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  const long long v0 = ((long long)blockIdx.x * CS_WAVES + (threadIdx.x >> 6)) * CS_T;
  if (v0 >= npad) return;                                            // wave-uniform; npad % 256 == 0
  const long long v = v0 + c;
  const cs_f16 acc = cs_tile(xp, npad, v, xp, npad, v, nq);
  // the diagonal (c, c) lives in lane half (c>>2)&1, register (c&3) + 4(c>>3)
  const int rd = (c & 3) + 4 * (c >> 3);
  float nv = 0.0f;
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (r == rd) nv = acc[r];
  if (h == ((c >> 2) & 1)) {
    norm[v] = nv;
    rnorm[v] = 1.0f / sqrtf(nv);                                     // correctly rounded sqrt and division
  }
  bool bad = false;                                                  // inf / nan: exponent all ones
  if (v < n) {
    for (int q = h; q < nq; q += 2) {
      const uint4 u = xp[(long long)q * npad + v];
      const u32 w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) bad |= (w[i] & 0x7C00u) == 0x7C00u || (w[i] & 0x7C000000u) == 0x7C000000u;
    }
  }
  if (bad) flags[0] = 1u;
}

// per-lane norms of the column this lane holds; zero past n
__device__ __forceinline__ void cs_col_norms(const float *__restrict__ nx, const float *__restrict__ rx, long long col, long long n,
                                             float &a, float &b) {
  a = col < n ? nx[col] : 0.0f;
  b = col < n ? rx[col] : 0.0f;
}

// (M, N) fp32 block: out[m * ldo + n] = distance (or similarity) of Y[m] and X[n] by epilogue E; a wave per 32 x 32 tile
template <class E>
__global__ __launch_bounds__(256) void pg_cos_dense_kernel(const uint4 *__restrict__ xp, const float *__restrict__ nx,
                                                           const float *__restrict__ rx, long long n, long long xnpad,
                                                           const uint4 *__restrict__ yp, const float *__restrict__ ny,
                                                           const float *__restrict__ ry, long long m, long long ynpad, int nq,
                                                           int similarity, float *__restrict__ out, long long ldo) {
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const long long x0 = ((long long)blockIdx.x * CS_WAVES + (threadIdx.x >> 6)) * CS_T;
  const long long y0 = (long long)blockIdx.y * CS_T;
  if (x0 >= n) return;                                               // wave-uniform
  const long long col = x0 + (lane & 31), yr = y0 + (lane & 31);
  const cs_f16 acc = cs_tile(xp, xnpad, col < n ? col : -1, yp, ynpad, yr < m ? yr : -1, nq);
  float ncol, rcol;
  cs_col_norms(nx, rx, col, n, ncol, rcol);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long long row = y0 + cs_row(r, h);
    if (row < m && col < n) out[row * ldo + col] = E::finish(acc[r], ncol, rcol, ny[row], ry[row], similarity);
  }
}

// Y row of row slot i of this wave: rows w*32 .. w*32+31, or row_list[w*32 + i] (restricted sweeps); -1 past the end
__device__ __forceinline__ long long cs_wave_row(int i, long long m, const long long *__restrict__ row_list, long long n_list) {
  const long long g = ((long long)blockIdx.x * CS_WAVES + (threadIdx.x >> 6)) * CS_T + i;
  if (!row_list) return g < m ? g : -1;
  if (g >= n_list) return -1;
  const long long r = row_list[g];
  return r >= 0 && r < m ? r : -1;
}

// ---- fused kNN: a wave owns 32 rows and sweeps all columns 32 at a time ----------------------------------------
// Row i's list is (lk[i], lc[i]): lane j = j-th smallest (key, column), and (tk[i], tc[i]) is its entry at rank
// `last` = the running threshold.  A tile value is a candidate only below the threshold of its register's row
// (one compare for most pairs); the candidates of a register go through a ballot and are inserted in lane order,
// by knn_insert (pg_select.h) into the list of row cs_row(r, 0) (lanes 0-31) or cs_row(r, 1) (lanes 32-63).

// FLOOR (pg_cosine_knn_round, first = 0): only pairs after each row's floor are candidates, rows written ldo elements
// apart.  The floors sit lane-per-row in one VGPR pair (lane i and i + 32: row slot i, the cs_wave_row order) and are
// read with readlane, instead of 32 more per-row values next to the lists.
template <class E, bool FLOOR>
__global__ __launch_bounds__(256) void pg_cos_knn_kernel(const uint4 *__restrict__ xp, const float *__restrict__ nx,
                                                         const float *__restrict__ rx, long long n, long long xnpad,
                                                         const uint4 *__restrict__ yp, const float *__restrict__ ny,
                                                         const float *__restrict__ ry, long long m, long long ynpad, int nq,
                                                         int similarity, int k, int first, int *__restrict__ idx,
                                                         float *__restrict__ w, const int *__restrict__ floor_idx,
                                                         const float *__restrict__ floor_w, long long floor_ld, long long ldo) {
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const long long yr = cs_wave_row(lane & 31, m, nullptr, 0);
  if (__builtin_amdgcn_readfirstlane((int)(cs_wave_row(0, m, nullptr, 0) < 0))) return;    // a wave past the end
  float nyv[16], ryv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long long row = cs_wave_row(cs_row(r, h), m, nullptr, 0);
    nyv[r] = row >= 0 ? ny[row] : 0.0f;
    ryv[r] = row >= 0 ? ry[row] : 0.0f;
  }
  const int last = first + k - 1;
  u32 lk[CS_T], lc[CS_T], tk[CS_T], tc[CS_T];
#pragma unroll
  for (int i = 0; i < CS_T; ++i) lk[i] = lc[i] = tk[i] = tc[i] = 0xFFFFFFFFu;
  u32 fkv = 0, fcv = 0;                                              // lane i: the floor of row slot i & 31
  if (FLOOR && yr >= 0) knn_floor(floor_idx[yr * floor_ld], cs_key(floor_w[yr * floor_ld], similarity), fkv, fcv);
  for (long long x0 = 0; x0 < n; x0 += CS_T) {
    const long long col = x0 + (lane & 31);
    const bool cok = col < n;
    const cs_f16 acc = cs_tile(xp, xnpad, cok ? col : -1, yp, ynpad, yr, nq);
    float ncol, rcol;
    cs_col_norms(nx, rx, col, n, ncol, rcol);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i0 = cs_row(r, 0), i1 = cs_row(r, 1);
      const u32 key = cs_key(E::finish(acc[r], ncol, rcol, nyv[r], ryv[r], similarity), similarity);
      const u32 thk = h ? tk[i1] : tk[i0], thc = h ? tc[i1] : tc[i0];
      bool cand = cok && (key < thk || (key == thk && (u32)col < thc));
      if (FLOOR) {
        const u32 f0k = __builtin_amdgcn_readlane(fkv, i0), f0c = __builtin_amdgcn_readlane(fcv, i0);
        const u32 f1k = __builtin_amdgcn_readlane(fkv, i1), f1c = __builtin_amdgcn_readlane(fcv, i1);
        cand = cand && knn_after(key, (u32)col, h ? f1k : f0k, h ? f1c : f0c);
      }
      const u64 mask = __builtin_amdgcn_ballot_w64(cand);
      if ((u32)mask) knn_insert(lk[i0], lc[i0], tk[i0], tc[i0], (u32)mask, key, 0, x0, last);
      if ((u32)(mask >> 32)) knn_insert(lk[i1], lc[i1], tk[i1], tc[i1], (u32)(mask >> 32), key, 32, x0, last);
    }
  }
#pragma unroll
  for (int i = 0; i < CS_T; ++i) {
    const long long row = cs_wave_row(i, m, nullptr, 0);
    if (row >= 0 && lane >= first && lane <= last) {
      const long long o = row * (FLOOR ? ldo : (long long)k) + (lane - first);
      const bool none = lc[i] == 0xFFFFFFFFu;
      idx[o] = none ? -1 : (int)lc[i];
      w[o] = none ? 0.0f : cs_unkey(lk[i], similarity);
    }
  }
}

// ---- fused epsilon selection.  Slot mode (row_list == NULL): every row's exact match count into counts[], its
// first `cap` matches (ascending columns) into its slot.  Fill mode: the rows of row_list only, every match written
// at indptr[row] (counts from a slot pass, so the segments fit).  A lane keeps the running count and output base of
// the row of each of its registers.
template <class E>
__global__ __launch_bounds__(256) void pg_cos_eps_kernel(const uint4 *__restrict__ xp, const float *__restrict__ nx,
                                                         const float *__restrict__ rx, long long n, long long xnpad,
                                                         const uint4 *__restrict__ yp, const float *__restrict__ ny,
                                                         const float *__restrict__ ry, long long m, long long ynpad, int nq,
                                                         int similarity, int cmp, float eps, const long long *__restrict__ row_list,
                                                         long long n_list, int cap, int *__restrict__ slot_idx,
                                                         float *__restrict__ slot_w, u32 *__restrict__ counts,
                                                         const long long *__restrict__ indptr, int *__restrict__ indices,
                                                         float *__restrict__ weights) {
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const long long yr = cs_wave_row(lane & 31, m, row_list, n_list);
  {
    const long long g0 = ((long long)blockIdx.x * CS_WAVES + (threadIdx.x >> 6)) * CS_T;
    if (g0 >= (row_list ? n_list : m)) return;                       // wave-uniform: a wave past the end
  }
  float nyv[16], ryv[16];
  long long base[16];
  u32 cnt[16];
  bool rok[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long long row = cs_wave_row(cs_row(r, h), m, row_list, n_list);
    rok[r] = row >= 0;
    nyv[r] = rok[r] ? ny[row] : 0.0f;
    ryv[r] = rok[r] ? ry[row] : 0.0f;
    base[r] = !rok[r] ? 0 : (row_list ? indptr[row] : row * (long long)cap);
    cnt[r] = 0;
  }
  for (long long x0 = 0; x0 < n; x0 += CS_T) {
    const long long col = x0 + (lane & 31);
    const bool cok = col < n;
    const cs_f16 acc = cs_tile(xp, xnpad, cok ? col : -1, yp, ynpad, yr, nq);
    float ncol, rcol;
    cs_col_norms(nx, rx, col, n, ncol, rcol);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float v = E::finish(acc[r], ncol, rcol, nyv[r], ryv[r], similarity);
      const bool hit = cok && rok[r] && pg_match(v, eps, cmp, similarity);
      const u64 mask = __builtin_amdgcn_ballot_w64(hit);
      if (!mask) continue;                                           // wave-uniform
      const u64 mine = h ? (mask & 0xFFFFFFFF00000000ull) : (mask & 0xFFFFFFFFull);
      if (hit) {
        const long long o = (long long)cnt[r] + mask_rank(mine);
        if (row_list) {
          indices[base[r] + o] = (int)col;
          weights[base[r] + o] = v;
        } else if (o < cap) {
          slot_idx[base[r] + o] = (int)col;
          slot_w[base[r] + o] = v;
        }
      }
      cnt[r] += (u32)__popcll(mine);
    }
  }
  if (!row_list && (lane & 31) == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long row = cs_wave_row(cs_row(r, h), m, nullptr, 0);
      if (row >= 0) counts[row] = cnt[r];
    }
  }
}

static int cs_nq(int d) { return (d + 7) / 8; }

static int cs_operands_bad(const void *xp, const float *xn, const float *xr, int64_t n, int64_t x_npad, const void *yp,
                           const float *yn, const float *yr, int64_t m, int64_t y_npad, int d) {
  return !xp || !xn || !xr || !yp || !yn || !yr || n <= 0 || m <= 0 || d <= 0 || x_npad < n || x_npad % 256 || y_npad < m;
}

// workgroups of CS_WAVES waves, a wave per 32 rows
static long long cs_groups(int64_t rows) { return (rows + CS_T * CS_WAVES - 1) / (CS_T * CS_WAVES); }

// "<entry>: <what>" as the error message of an argument check
static int cs_bad(const char *entry, const char *what) {
  char buf[160];
  snprintf(buf, sizeof(buf), "%s: %s", entry, what);
  return pg_fail(PG_E_BADARG, buf);
}

// The bodies of the pg_cosine_* / pg_euclidean_* entries: the argument checks and the launch of epilogue E's instance.
template <class E>
static int cs_dense(const char *entry, const void *x_packed, const float *x_norms, const float *x_rnorms, int64_t n,
                    int64_t x_npad, const void *y_packed, const float *y_norms, const float *y_rnorms, int64_t m,
                    int64_t y_npad, int d, int similarity, float *out, int64_t ldo, void *stream) {
  if (cs_operands_bad(x_packed, x_norms, x_rnorms, n, x_npad, y_packed, y_norms, y_rnorms, m, y_npad, d) || !out || ldo < n)
    return cs_bad(entry, "bad argument");
  if ((m + CS_T - 1) / CS_T > 65535 || cs_groups(n) > 0x7FFFFFFFll) return cs_bad(entry, "m too large for one launch");
  const dim3 grid((unsigned)cs_groups(n), (unsigned)((m + CS_T - 1) / CS_T));
  pg_cos_dense_kernel<E><<<grid, dim3(64 * CS_WAVES), 0, (hipStream_t)stream>>>(
      (const uint4 *)x_packed, x_norms, x_rnorms, n, x_npad, (const uint4 *)y_packed, y_norms, y_rnorms, m, y_npad, cs_nq(d),
      similarity ? 1 : 0, out, ldo);
  return pg_launched(entry);
}

template <class E>
static int cs_knn(const char *entry, const void *x_packed, const float *x_norms, const float *x_rnorms, int64_t n,
                  int64_t x_npad, const void *y_packed, const float *y_norms, const float *y_rnorms, int64_t m, int64_t y_npad,
                  int d, int similarity, int k, int first, int32_t *idx_out, float *w_out, void *stream) {
  if (cs_operands_bad(x_packed, x_norms, x_rnorms, n, x_npad, y_packed, y_norms, y_rnorms, m, y_npad, d) || !idx_out || !w_out)
    return cs_bad(entry, "bad argument");
  if (k < 1 || first < 0 || first + k > 64) return cs_bad(entry, "first + k must be at most 64");
  if (n > 0x7FFFFFFFll || cs_groups(m) > 0x7FFFFFFFll) return cs_bad(entry, "too many vectors for one launch");
  pg_cos_knn_kernel<E, false><<<dim3((unsigned)cs_groups(m)), dim3(64 * CS_WAVES), 0, (hipStream_t)stream>>>(
      (const uint4 *)x_packed, x_norms, x_rnorms, n, x_npad, (const uint4 *)y_packed, y_norms, y_rnorms, m, y_npad, cs_nq(d),
      similarity ? 1 : 0, k, first, idx_out, w_out, nullptr, nullptr, 0, k);
  return pg_launched(entry);
}

template <class E>
static int cs_knn_round(const char *entry, const void *x_packed, const float *x_norms, const float *x_rnorms, int64_t n,
                        int64_t x_npad, const void *y_packed, const float *y_norms, const float *y_rnorms, int64_t m,
                        int64_t y_npad, int d, int similarity, int k, const int32_t *floor_idx, const float *floor_w,
                        int64_t floor_ld, int32_t *idx_out, float *w_out, int64_t ldo, void *stream) {
  if (cs_operands_bad(x_packed, x_norms, x_rnorms, n, x_npad, y_packed, y_norms, y_rnorms, m, y_npad, d) || !idx_out || !w_out ||
      !floor_idx || !floor_w || floor_ld < 0 || ldo < k)
    return cs_bad(entry, "bad argument");
  if (k < 1 || k > 64) return cs_bad(entry, "k must be 1..64");
  if (n > 0x7FFFFFFFll || cs_groups(m) > 0x7FFFFFFFll) return cs_bad(entry, "too many vectors for one launch");
  pg_cos_knn_kernel<E, true><<<dim3((unsigned)cs_groups(m)), dim3(64 * CS_WAVES), 0, (hipStream_t)stream>>>(
      (const uint4 *)x_packed, x_norms, x_rnorms, n, x_npad, (const uint4 *)y_packed, y_norms, y_rnorms, m, y_npad, cs_nq(d),
      similarity ? 1 : 0, k, 0, idx_out, w_out, floor_idx, floor_w, floor_ld, ldo);
  return pg_launched(entry);
}

template <class E>
static int cs_eps_slots(const char *entry, const void *x_packed, const float *x_norms, const float *x_rnorms, int64_t n,
                        int64_t x_npad, const void *y_packed, const float *y_norms, const float *y_rnorms, int64_t m,
                        int64_t y_npad, int d, int similarity, int cmp, float eps, int cap, int32_t *slot_idx, float *slot_w,
                        uint32_t *counts, void *stream) {
  if (cs_operands_bad(x_packed, x_norms, x_rnorms, n, x_npad, y_packed, y_norms, y_rnorms, m, y_npad, d) || !slot_idx ||
      !slot_w || !counts || cap < 1 || pg_cmp_bad(cmp))
    return cs_bad(entry, "bad argument");
  if (n > 0x7FFFFFFFll || cs_groups(m) > 0x7FFFFFFFll) return cs_bad(entry, "too many vectors for one launch");
  pg_cos_eps_kernel<E><<<dim3((unsigned)cs_groups(m)), dim3(64 * CS_WAVES), 0, (hipStream_t)stream>>>(
      (const uint4 *)x_packed, x_norms, x_rnorms, n, x_npad, (const uint4 *)y_packed, y_norms, y_rnorms, m, y_npad, cs_nq(d),
      similarity ? 1 : 0, cmp, eps, nullptr, 0, cap, slot_idx, slot_w, counts, nullptr, nullptr, nullptr);
  return pg_launched(entry);
}

template <class E>
static int cs_eps_fill_rows(const char *entry, const void *x_packed, const float *x_norms, const float *x_rnorms, int64_t n,
                            int64_t x_npad, const void *y_packed, const float *y_norms, const float *y_rnorms, int64_t m,
                            int64_t y_npad, int d, int similarity, int cmp, float eps, const int64_t *row_list, int64_t n_list,
                            const int64_t *indptr, int32_t *indices, float *weights, void *stream) {
  if (cs_operands_bad(x_packed, x_norms, x_rnorms, n, x_npad, y_packed, y_norms, y_rnorms, m, y_npad, d) || !row_list ||
      n_list <= 0 || !indptr || !indices || !weights || pg_cmp_bad(cmp))
    return cs_bad(entry, "bad argument");
  if (n > 0x7FFFFFFFll || cs_groups(n_list) > 0x7FFFFFFFll) return cs_bad(entry, "too many vectors for one launch");
  pg_cos_eps_kernel<E><<<dim3((unsigned)cs_groups(n_list)), dim3(64 * CS_WAVES), 0, (hipStream_t)stream>>>(
      (const uint4 *)x_packed, x_norms, x_rnorms, n, x_npad, (const uint4 *)y_packed, y_norms, y_rnorms, m, y_npad, cs_nq(d),
      similarity ? 1 : 0, cmp, eps, (const long long *)row_list, n_list, 1, nullptr, nullptr, nullptr,
      (const long long *)indptr, indices, weights);
  return pg_launched(entry);
}

extern "C" {

int pg_cosine_prep(const void *packed, int64_t n, int64_t npad, int d, float *norms, float *rnorms, uint32_t *flags,
                   void *stream) {
  if (!packed || !norms || !rnorms || !flags || n < 0 || d <= 0 || npad < n || npad <= 0 || npad % 256)
    return pg_fail(PG_E_BADARG, "pg_cosine_prep: bad argument");
  pg_cos_prep_kernel<<<dim3((unsigned)(npad / (CS_T * CS_WAVES))), dim3(64 * CS_WAVES), 0, (hipStream_t)stream>>>(
      (const uint4 *)packed, n, npad, cs_nq(d), norms, rnorms, flags);
  return pg_launched("pg_cos_prep_kernel");
}

// One argument list per entry, shared by the two metrics (include/prograph_hip.h).
#define CS_ENTRIES(METRIC, E)                                                                                              \
  int pg_##METRIC##_dense(CS_OPS, float *out, int64_t ldo, void *stream) {                                                 \
    return cs_dense<E>("pg_" #METRIC "_dense", CS_OPA, out, ldo, stream);                                                  \
  }                                                                                                                        \
  int pg_##METRIC##_knn(CS_OPS, int k, int first, int32_t *idx_out, float *w_out, void *stream) {                          \
    return cs_knn<E>("pg_" #METRIC "_knn", CS_OPA, k, first, idx_out, w_out, stream);                                      \
  }                                                                                                                        \
  int pg_##METRIC##_knn_round(CS_OPS, int k, const int32_t *floor_idx, const float *floor_w, int64_t floor_ld,             \
                              int32_t *idx_out, float *w_out, int64_t ldo, void *stream) {                                 \
    return cs_knn_round<E>("pg_" #METRIC "_knn_round", CS_OPA, k, floor_idx, floor_w, floor_ld, idx_out, w_out, ldo,       \
                           stream);                                                                                        \
  }                                                                                                                        \
  int pg_##METRIC##_eps_slots(CS_OPS, int cmp, float eps, int cap, int32_t *slot_idx, float *slot_w, uint32_t *counts,     \
                              void *stream) {                                                                              \
    return cs_eps_slots<E>("pg_" #METRIC "_eps_slots", CS_OPA, cmp, eps, cap, slot_idx, slot_w, counts, stream);           \
  }                                                                                                                        \
  int pg_##METRIC##_eps_fill_rows(CS_OPS, int cmp, float eps, const int64_t *row_list, int64_t n_list,                     \
                                  const int64_t *indptr, int32_t *indices, float *weights, void *stream) {                 \
    return cs_eps_fill_rows<E>("pg_" #METRIC "_eps_fill_rows", CS_OPA, cmp, eps, row_list, n_list, indptr, indices,        \
                               weights, stream);                                                                           \
  }
#define CS_OPS                                                                                                     \
  const void *x_packed, const float *x_norms, const float *x_rnorms, int64_t n, int64_t x_npad, const void *y_packed, \
      const float *y_norms, const float *y_rnorms, int64_t m, int64_t y_npad, int d, int similarity
#define CS_OPA x_packed, x_norms, x_rnorms, n, x_npad, y_packed, y_norms, y_rnorms, m, y_npad, d, similarity

CS_ENTRIES(cosine, cs_cosine)
CS_ENTRIES(euclidean, cs_euclid)       // the Euclidean instances ignore x_rnorms / y_rnorms (they must still be given)

// metric-free: the Euclidean slots go through this entry too
int pg_cosine_eps_compact(int64_t m, int cap, const int32_t *slot_idx, const float *slot_w, const uint32_t *counts,
                          const int64_t *indptr, int32_t *indices, float *weights, void *stream) {
  return pg_eps_compact_launch<float>("pg_cosine_eps_compact", m, cap, slot_idx, slot_w, counts, indptr, indices, weights, stream);
}

}  // extern "C"
