// The selection of pg_f16_knn / pg_f16_eps_* (pg_mink.hip) on blocks of 32-bit integers: what the alignment kernels beyond
// 128 positions (pg_aln_long.hip) write, whose values are no fp16 integers.  The same structure: one wave per row, 64
// columns per ballot, the kNN list in one VGPR pair (knn_insert, pg_select.h), the stable (key, column) order.  Values
// are non-negative int32, so the key is the value itself, or 0x7FFFFFFF - value for a descending order; both stay below
// the 0xFFFFFFFF that marks an empty list entry.
#include "pg_select.h"

__device__ __forceinline__ u32 si_key(int v, int descending) { return descending ? 0x7FFFFFFFu - (u32)v : (u32)v; }

// ranks first .. first+k-1 of every row's (key, column) order.  FLOOR (pg_i32_knn_round, first = 0): only pairs after the
// row's floor (knn_floor) are candidates, and rows are written ldo elements apart; the floor is the previous round's last
// entry, whose value gives its key back.
template <bool FLOOR>
__global__ __launch_bounds__(256) void pg_i32_knn_kernel(const int *__restrict__ vals, long long m, long long n, long long ld, int k,
                                                         int first, int descending, int *__restrict__ idx, int *__restrict__ w,
                                                         const int *__restrict__ floor_idx, const int *__restrict__ floor_w,
                                                         long long floor_ld, long long ldo) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= m) return;
  const int *d = vals + row * ld;
  u32 lk = 0xFFFFFFFFu, lc = 0xFFFFFFFFu;                 // lane j = j-th smallest (key, column)
  const int last = first + k - 1;
  u32 tk = 0xFFFFFFFFu, tc = 0xFFFFFFFFu;                 // current entry of lane `last`
  u32 fk = 0, fc = 0;
  if (FLOOR) knn_floor(floor_idx[row * floor_ld], si_key(floor_w[row * floor_ld], descending), fk, fc);
  for (long long c0 = 0; c0 < n; c0 += 64) {
    const long long c = c0 + lane;
    const u32 key = c < n ? si_key(d[c], descending) : 0xFFFFFFFFu;
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

// comp(v, thr) & (v > 0); cmp | PG_CMP_KEEP_ZERO: comp(v, thr) & (v >= 0) - pg_match's distance form on integers
__device__ __forceinline__ bool si_match(long long v, long long thr, int cmp) {
  bool ok;
  switch (cmp & ~PG_CMP_KEEP_ZERO) {
    case PG_CMP_LE: ok = v <= thr; break;
    case PG_CMP_LT: ok = v < thr; break;
    case PG_CMP_EQ: ok = v == thr; break;
    case PG_CMP_GE: ok = v >= thr; break;
    default: ok = v > thr; break;
  }
  return ok && ((cmp & PG_CMP_KEEP_ZERO) ? v >= 0 : v > 0);
}

// epsilon selection on an integer block: count, or fill at indptr
__global__ __launch_bounds__(256) void pg_i32_eps_kernel(const int *__restrict__ vals, long long m, long long n, long long ld, int cmp,
                                                         long long thr, u32 *__restrict__ counts, const long long *__restrict__ indptr,
                                                         int *__restrict__ indices, int *__restrict__ weights) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= m) return;
  const int *d = vals + row * ld;
  long long run = indptr ? indptr[row] : 0;
  u32 cnt = 0;
  for (long long c0 = 0; c0 < n; c0 += 64) {
    const long long c = c0 + lane;
    const int v = c < n ? d[c] : 0;
    const bool hit = c < n && si_match(v, thr, cmp);
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

extern "C" {

int pg_i32_knn(const int32_t *vals, int64_t m, int64_t n, int64_t ld, int k, int first, int descending, int32_t *idx_out,
               int32_t *w_out, void *stream) {
  if (!vals || !idx_out || !w_out || m <= 0 || n <= 0 || ld < n) return pg_fail(PG_E_BADARG, "pg_i32_knn: bad argument");
  if (k < 1 || first < 0 || first + k > 64) return pg_fail(PG_E_BADARG, "pg_i32_knn: first + k must be at most 64");
  pg_i32_knn_kernel<false><<<dim3((unsigned)((m + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(
      vals, m, n, ld, k, first, descending, idx_out, w_out, nullptr, nullptr, 0, 0);
  return pg_launched("pg_i32_knn_kernel");
}

int pg_i32_knn_round(const int32_t *vals, int64_t m, int64_t n, int64_t ld, int k, int descending, const int32_t *floor_idx,
                     const int32_t *floor_w, int64_t floor_ld, int32_t *idx_out, int32_t *w_out, int64_t ldo, void *stream) {
  if (!vals || !idx_out || !w_out || !floor_idx || !floor_w || m <= 0 || n <= 0 || ld < n || floor_ld < 1 || ldo < k)
    return pg_fail(PG_E_BADARG, "pg_i32_knn_round: bad argument");
  if (k < 1 || k > 64) return pg_fail(PG_E_BADARG, "pg_i32_knn_round: k must be 1..64");
  pg_i32_knn_kernel<true><<<dim3((unsigned)((m + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(
      vals, m, n, ld, k, 0, descending, idx_out, w_out, floor_idx, floor_w, floor_ld, ldo);
  return pg_launched("pg_i32_knn_kernel(round)");
}

int pg_i32_eps_count(const int32_t *vals, int64_t m, int64_t n, int64_t ld, int cmp, int64_t thr, uint32_t *counts, void *stream) {
  if (!vals || !counts || m <= 0 || n <= 0 || ld < n || pg_cmp_bad(cmp)) return pg_fail(PG_E_BADARG, "pg_i32_eps_count: bad argument");
  pg_i32_eps_kernel<<<dim3((unsigned)((m + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(vals, m, n, ld, cmp, thr, counts, nullptr,
                                                                                         nullptr, nullptr);
  return pg_launched("pg_i32_eps_kernel(count)");
}

int pg_i32_eps_fill(const int32_t *vals, int64_t m, int64_t n, int64_t ld, int cmp, int64_t thr, const int64_t *indptr,
                    int32_t *indices, int32_t *weights, void *stream) {
  if (!vals || !indptr || !indices || !weights || m <= 0 || n <= 0 || ld < n || pg_cmp_bad(cmp))
    return pg_fail(PG_E_BADARG, "pg_i32_eps_fill: bad argument");
  pg_i32_eps_kernel<<<dim3((unsigned)((m + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(
      vals, m, n, ld, cmp, thr, nullptr, (const long long *)indptr, indices, weights);
  return pg_launched("pg_i32_eps_kernel(fill)");
}

}  // extern "C"
