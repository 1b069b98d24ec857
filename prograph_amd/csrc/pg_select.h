// The selection layer of the fp16, Minkowski and cosine paths (pg_mink.hip, pg_cos.hip): what turns a row's values
// into its kNN list or its CSR entries, whatever computed the values.
#pragma once
#include "pg_common.h"
#include "../../include/prograph_hip.h"

// cmp of the eps entries: one of the five codes, with or without PG_CMP_KEEP_ZERO
static inline bool pg_cmp_bad(int cmp) { return (cmp & ~PG_CMP_KEEP_ZERO) < PG_CMP_LE || (cmp & ~PG_CMP_KEEP_ZERO) > PG_CMP_GT; }

// epsilon test of a distance / similarity v
//   distances:    comp(d, eps) & (d > 0)      (prograph.py:736)
//   similarities: comp(eps, s) & (s < 1)      (:734), eps already 1/(1+eps) rounded like the values
//   cmp | PG_CMP_KEEP_ZERO: without the second test (queries: a vector equal to the query is a hit)
__device__ __forceinline__ bool pg_match(float v, float eps, int cmp, int similarity) {
  const float a = similarity ? eps : v, b = similarity ? v : eps;
  bool ok;
  switch (cmp & ~PG_CMP_KEEP_ZERO) {
    case PG_CMP_LE: ok = a <= b; break;
    case PG_CMP_LT: ok = a < b; break;
    case PG_CMP_EQ: ok = a == b; break;
    case PG_CMP_GE: ok = a >= b; break;
    default: ok = a > b; break;
  }
  return ok && ((cmp & PG_CMP_KEEP_ZERO) || (similarity ? v < 1.0f : v > 0.0f));
}

// A row's kNN list is one VGPR pair (lk, lc): lane j = its j-th smallest (key, column); (tk, tc) is the entry of lane
// `last`, the running threshold (wave-uniform).  Inserts the candidates of `mask` in bit order: bit b is the value
// `key` of lane b + boff, column x0 + b.  Mask: u64 (a ballot) or u32 (one half of it, boff = 0 / 32).
template <typename Mask>
__device__ __forceinline__ void knn_insert(u32 &lk, u32 &lc, u32 &tk, u32 &tc, Mask mask, u32 key, int boff, long long x0,
                                           int last) {
  while (mask) {
    int b;
    if constexpr (sizeof(Mask) == 8) b = __builtin_ctzll(mask);
    else b = __builtin_ctz(mask);
    mask &= mask - 1;
    const u32 xk = __builtin_amdgcn_readlane(key, b + boff), xc = (u32)(x0 + b);
    if (xk < tk || (xk == tk && xc < tc)) {
      const bool keep = lk < xk || (lk == xk && lc <= xc);           // entries not after x stay
      const u32 pk = wave_shr1(lk, 0u), pc = wave_shr1(lc, 0u);
      const bool prev_after = pk > xk || (pk == xk && pc > xc);      // lane-1's entry also moves: take it, else x lands here
      lk = keep ? lk : (prev_after ? pk : xk);
      lc = keep ? lc : (prev_after ? pc : xc);
      tk = __builtin_amdgcn_readlane(lk, last);
      tc = __builtin_amdgcn_readlane(lc, last);
    }
  }
}

// slots -> CSR for the rows that kept all their matches (count <= cap); one wave per row.  The rows beyond their
// slot are written by the metric's fill_rows sweep.
template <typename W>
__global__ __launch_bounds__(256) void pg_eps_compact_kernel(long long m, int cap, const int *__restrict__ slot_idx,
                                                             const W *__restrict__ slot_w, const u32 *__restrict__ counts,
                                                             const long long *__restrict__ indptr, int *__restrict__ indices,
                                                             W *__restrict__ weights) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= m) return;
  const u32 cnt = counts[row];
  if (cnt > (u32)cap) return;
  const long long o = indptr[row], s = row * (long long)cap;
  for (u32 i = lane; i < cnt; i += 64) {
    indices[o + i] = slot_idx[s + i];
    weights[o + i] = slot_w[s + i];
  }
}

// the exported compact entry of a metric: argument check and launch
template <typename W>
static int pg_eps_compact_launch(const char *name, int64_t m, int cap, const int32_t *slot_idx, const void *slot_w,
                                 const uint32_t *counts, const int64_t *indptr, int32_t *indices, void *weights, void *stream) {
  if (!slot_idx || !slot_w || !counts || !indptr || !indices || !weights || m <= 0 || cap < 1) {
    char buf[96];
    snprintf(buf, sizeof(buf), "%s: bad argument", name);
    return pg_fail(PG_E_BADARG, buf);
  }
  pg_eps_compact_kernel<W><<<dim3((unsigned)((m + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(
      m, cap, slot_idx, (const W *)slot_w, counts, (const long long *)indptr, indices, (W *)weights);
  return pg_launched("pg_eps_compact_kernel");
}
